"""numpy statements of the hybrid search for the tests; they live in tests/ only and the product never falls back to
them.

* ``pack`` -- the stored form of raw CSR tokens (distinct terms ascending, counts saturated at 255, raw lengths), by ONE
  sort of (row, term) keys: independent of the library's per-row sort-and-count.
* ``bm25_f32`` -- the float32 restatement of the device arithmetic of ``include/css_hip.h``, operation for operation,
  the sum in QUERY-TERM order; ``bm25_f64`` -- the same formula in float64 (the truth of the value checks).
* ``FakeLexIndex`` -- ``prior_fakes.FakePriorIndex`` plus term lists: the TEST DOUBLE of the device index for the CPU
  tests of ``HybridStorage.search_hybrid`` and the sharded ``search_hybrid``.  Every value in fp64 and ONE ``lexsort``
  by (value, id); no sweep, no column kernel, no merge.

Callers that compare a sharded with an unsharded double build the rows from multiples of 1/8; the lexical value of a
row is a function of its own list and the call's constants, so it has the same fp64 bits wherever the row lives."""
import numpy as np

from prior_fakes import FakePriorIndex
from related_fakes import FLT_MAX

TERM_SPACE = 1 << 24


def pack(off, tok):
    """(offsets, terms uint32, tfs uint8, dl uint32) of CSR raw tokens."""
    off = np.asarray(off, np.int64)
    n = off.shape[0] - 1
    dl = np.diff(off).astype(np.uint32)
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(off))
    key, cnt = np.unique(rows << 24 | np.asarray(tok, np.int64), return_counts=True)
    poff = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(key >> 24, minlength=n), out=poff[1:])
    return poff, (key & (TERM_SPACE - 1)).astype(np.uint32), np.minimum(cnt, 255).astype(np.uint8), dl


def _hits(poff, terms, t):
    hit = np.flatnonzero(terms == np.uint32(t))
    return hit, np.searchsorted(poff, hit, side="right") - 1


def bm25_f32(poff, terms, tfs, dl, qterms, weights, k1, b, avgdl, hits=_hits):
    f = np.float32
    k1, b, avgdl = f(k1), f(b), f(avgdl)
    w = np.asarray(weights, np.float32)
    c0 = f(k1 * f(f(1.0) - b))
    c1 = f(f(k1 * b) / avgdl)
    K = (c0 + (c1 * np.asarray(dl).astype(np.float32)).astype(np.float32)).astype(np.float32)
    k1p = f(k1 + f(1.0))
    lex = np.zeros(poff.shape[0] - 1, np.float32)
    for j, t in enumerate(qterms):
        hit, r = hits(poff, terms, t)
        tf = tfs[hit].astype(np.float32)
        g = ((tf * k1p).astype(np.float32) / (tf + K[r]).astype(np.float32)).astype(np.float32)
        lex[r] = (lex[r] + (w[j] * g).astype(np.float32)).astype(np.float32)
    return lex


def bm25_f64(poff, terms, tfs, dl, qterms, weights, k1, b, avgdl, hits=_hits):
    """float64 throughout, from the float32 weights and constants the call receives (widened exactly)."""
    f = lambda v: np.float64(np.float32(v))   # noqa: E731
    k1, b, avgdl = f(k1), f(b), f(avgdl)
    w = np.asarray(weights, np.float32).astype(np.float64)
    K = k1 * (1.0 - b) + (k1 * b / avgdl) * np.asarray(dl).astype(np.float64)
    lex = np.zeros(poff.shape[0] - 1, np.float64)
    for j, t in enumerate(qterms):
        hit, r = hits(poff, terms, t)
        tf = tfs[hit].astype(np.float64)
        lex[r] += w[j] * (tf * (k1 + 1.0)) / (tf + K[r])
    return lex


class FakeLexIndex(FakePriorIndex):
    def __init__(self, d, metric=0, device=0):
        super().__init__(d, metric, device)
        self._lists = []   # per leading row: (sorted distinct terms, saturated counts, raw length)

    def set_terms(self, lists, row0=None):
        if isinstance(lists, tuple):
            off, tok = lists
            lists = [np.asarray(tok[off[i]:off[i + 1]]) for i in range(len(off) - 1)]
        row0 = len(self._lists) if row0 is None else int(row0)
        assert 0 <= row0 <= len(self._lists) and row0 + len(lists) <= self.ntotal
        self.calls.append(("set_terms", row0, len(lists)))
        del self._lists[row0:]
        for r in lists:
            r = np.asarray(r, np.int64).reshape(-1)
            assert r.size == 0 or (r.min() >= 0 and r.max() < TERM_SPACE)
            t, c = np.unique(r, return_counts=True)
            self._lists.append((t, np.minimum(c, 255), int(r.size)))

    def term_stats(self, terms):
        t = np.asarray(terms, np.int64).reshape(-1)
        df = np.array([sum(int(q in set(l[0].tolist())) for l in self._lists) for q in t], np.int64).reshape(-1)
        return df, self.ntotal, sum(l[2] for l in self._lists)

    def _lex(self, terms, weights, k1, b, avgdl):
        lex = np.zeros(self.ntotal, np.float64)
        for r, (t, c, dl) in enumerate(self._lists):
            K = k1 * (1.0 - b) + k1 * b * dl / avgdl
            for q, w in zip(terms, weights):
                at = np.flatnonzero(t == q)
                if at.size:
                    tf = float(c[at[0]])
                    lex[r] += float(w) * tf * (k1 + 1.0) / (tf + K)
        return lex

    def search_hybrid(self, q, terms, weights, k, alpha, k1=1.2, b=0.75, avgdl=None, normalize=False, allow=None):
        k = int(k)
        terms = [int(t) for t in np.asarray(terms, np.int64).reshape(-1)]
        weights = np.asarray(weights, np.float32).reshape(-1)
        self.calls.append(("search_hybrid", k, allow is not None, tuple(terms)))
        assert 1 <= k <= 128 and np.isfinite(alpha) and len(terms) == weights.shape[0] <= 32 and len(set(terms)) == len(terms)
        if avgdl is None:
            _, n, total = self.term_stats(())
            avgdl = total / n if n and total else 1.0
        q64 = np.asarray(q, np.float64).reshape(1, self.d)
        x64 = self._x.astype(np.float64)
        lex = self._lex(terms, weights, float(k1), float(b), float(np.float32(avgdl)))
        if self.metric_type == 0:
            s = (q64 @ x64.T)[0]
            f = s + float(alpha) * lex
        else:
            s = ((q64 - x64) ** 2).sum(-1)
            f = s - float(alpha) * lex
        ids = np.flatnonzero(self._ok(1, allow)[0])
        order = ids[np.lexsort((ids, -f[ids] if self.metric_type == 0 else f[ids]))][:k]
        pad = -FLT_MAX if self.metric_type == 0 else FLT_MAX
        D, I = np.full((1, k), pad, np.float32), np.full((1, k), -1, np.int64)
        S, L = np.full((1, k), pad, np.float32), np.zeros((1, k), np.float32)
        D[0, :order.size], S[0, :order.size], L[0, :order.size], I[0, :order.size] = f[order], s[order], lex[order], order + self.base
        return D, I, S, L


class Lists:
    """Raw CSR lists with their stored form and an inverted order, so that the columns of many queries cost one sort."""

    def __init__(self, off, tok):
        self.off, self.tok = np.asarray(off, np.int64), np.asarray(tok, np.uint32)
        self.poff, self.terms, self.tfs, self.dl = pack(self.off, self.tok)
        self.n = self.off.shape[0] - 1
        self._erow = np.repeat(np.arange(self.n), np.diff(self.poff))
        self._order = np.argsort(self.terms, kind="stable")
        self._sorted = self.terms[self._order]

    def hits(self, poff, terms, t):
        a, e = np.searchsorted(self._sorted, [np.uint32(t), np.uint32(t) + np.uint64(1)])
        hit = self._order[a:e]
        return hit, self._erow[hit]

    def df(self, terms):
        t = np.asarray(terms, np.int64).reshape(-1)
        return (np.searchsorted(self._sorted, t + 1) - np.searchsorted(self._sorted, t)).astype(np.int64)

    @property
    def total_len(self):
        return int(self.dl.astype(np.int64).sum())

    def avgdl(self):
        return float(np.float32(self.total_len / self.n)) if self.total_len else 1.0

    def f32(self, qterms, weights, k1, b, avgdl):
        return bm25_f32(self.poff, self.terms, self.tfs, self.dl, qterms, weights, k1, b, avgdl, hits=self.hits)

    def f64(self, qterms, weights, k1, b, avgdl):
        return bm25_f64(self.poff, self.terms, self.tfs, self.dl, qterms, weights, k1, b, avgdl, hits=self.hits)

    def rows(self, sel):
        """The lists of the selected rows (a boolean mask or row numbers), in that order, as a new ``Lists``."""
        sel = np.flatnonzero(sel) if np.asarray(sel).dtype == np.bool_ else np.asarray(sel, np.int64)
        lens = np.diff(self.off)[sel]
        noff = np.zeros(sel.shape[0] + 1, np.int64)
        np.cumsum(lens, out=noff[1:])
        src = np.repeat(self.off[:-1][sel] - noff[:-1], lens) + np.arange(int(noff[-1]))
        return Lists(noff, self.tok[src])
