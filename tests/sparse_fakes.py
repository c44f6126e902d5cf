"""numpy statements of the sparse-vector side of the flat index for the tests; they live in tests/ only and the product
never falls back to them.

* ``Vectors`` -- CSR sparse vectors with their stored form (per row ascending by term, by ONE sort of (row, term) keys:
  independent of the library's per-row sort) and an inverted order, so that the columns of many queries cost one sort.
  ``f32`` is the float32 restatement of the device arithmetic of ``include/css_hip.h``, operation for operation, the
  sum in QUERY-TERM order, with the hit flags; ``f64`` the same sum in float64 from the float32 inputs (widened
  exactly), with ``sum_j |w_j d_j|`` for the error bound.
* ``topk`` -- the pure sparse ranking: hit and allowed rows by ONE ``lexsort`` on (value descending, id ascending).
* ``topk_slice`` -- the launch geometry of the column top-k (rows per block), restated from the constants that
  ``_native`` mirrors from ``csrc/css_sparse.h``.
* ``FakeSparseIndex`` -- ``prior_fakes.FakePriorIndex`` plus sparse vectors: the TEST DOUBLE of the device index for the
  CPU tests of the sharded ``search_sparse`` / ``search_hybrid_sparse``.  Every value in fp64 and ONE ``lexsort``."""
import numpy as np

from prior_fakes import FakePriorIndex
from related_fakes import FLT_MAX

TERM_SPACE = 1 << 24


class Vectors:
    def __init__(self, off, terms, weights):
        off = np.asarray(off, np.int64)
        terms, weights = np.asarray(terms, np.uint32), np.asarray(weights, np.float32)
        self.n = off.shape[0] - 1
        rows = np.repeat(np.arange(self.n, dtype=np.int64), np.diff(off))
        order = np.argsort(rows << 24 | terms.astype(np.int64), kind="stable")
        self.off, self.terms, self.w = off, np.ascontiguousarray(terms[order]), np.ascontiguousarray(weights[order])
        self._erow = rows                                      # (the sort keeps the rows: row is the major key)
        self._order = np.argsort(self.terms, kind="stable")
        self._sorted = self.terms[self._order]

    def hits(self, t):
        a, e = np.searchsorted(self._sorted, [np.uint32(t), np.uint32(t) + np.uint64(1)])
        hit = self._order[a:e]
        return hit, self._erow[hit]

    def f32(self, qterms, qweights):
        """(sp float32 [n], hit bool [n]): sp_r = sp_r + w_j * d for j in the caller's order, float32 throughout."""
        w = np.asarray(qweights, np.float32)
        sp, hit = np.zeros(self.n, np.float32), np.zeros(self.n, bool)
        for j, t in enumerate(qterms):
            e, r = self.hits(t)
            sp[r] = (sp[r] + (w[j] * self.w[e]).astype(np.float32)).astype(np.float32)
            hit[r] = True
        return sp, hit

    def f64(self, qterms, qweights):
        """(sp float64 [n], sum_j |w_j d_j| float64 [n]) from the float32 inputs."""
        w = np.asarray(qweights, np.float32).astype(np.float64)
        sp, mag = np.zeros(self.n, np.float64), np.zeros(self.n, np.float64)
        for j, t in enumerate(qterms):
            e, r = self.hits(t)
            p = w[j] * self.w[e].astype(np.float64)
            sp[r] += p
            mag[r] += np.abs(p)
        return sp, mag

    def rows(self, sel):
        """The vectors of the selected rows (a boolean mask or row numbers), in that order, as a new ``Vectors``."""
        sel = np.flatnonzero(sel) if np.asarray(sel).dtype == np.bool_ else np.asarray(sel, np.int64)
        lens = np.diff(self.off)[sel]
        noff = np.zeros(sel.shape[0] + 1, np.int64)
        np.cumsum(lens, out=noff[1:])
        src = np.repeat(self.off[:-1][sel] - noff[:-1], lens) + np.arange(int(noff[-1]))
        return Vectors(noff, self.terms[src], self.w[src])

    def padded(self, n):
        """The same vectors on an index of n >= self.n rows: the rows behind them are empty."""
        return Vectors(np.concatenate([self.off, np.full(n - self.n, self.off[-1])]), self.terms, self.w)

    @property
    def csr(self):
        return self.off, self.terms, self.w


def topk(sp, hit, k, allowed=None, id_base=0):
    """(D float32 [1, k], I int64 [1, k]) of the pure sparse search from a column and its hit flags."""
    ok = hit if allowed is None else hit & np.asarray(allowed, bool)
    ids = np.flatnonzero(ok)
    order = ids[np.lexsort((ids, -sp[ids].astype(np.float64)))][:k]
    D, I = np.full((1, k), -FLT_MAX, np.float32), np.full((1, k), -1, np.int64)
    D[0, :order.size], I[0, :order.size] = sp[order], order + id_base
    return D, I


def topk_slice(n):
    from claude_semantic_search_amd import _native as nat

    per = -(-n // nat.SPARSE_TOPK_MAX_PARTS)
    return max(nat.SPARSE_TOPK_MIN_SLICE, -(-per // 256) * 256)


class FakeSparseIndex(FakePriorIndex):
    def __init__(self, d, metric=0, device=0):
        super().__init__(d, metric, device)
        self._vecs = []   # per leading row: (terms ascending, weights)

    @property
    def sparse_rows(self):
        return len(self._vecs)

    def set_sparse(self, vectors, row0=None):
        if isinstance(vectors, tuple) and len(vectors) == 3 and isinstance(vectors[0], np.ndarray):
            off, t, w = vectors
            vectors = [(np.asarray(t[off[i]:off[i + 1]]), np.asarray(w[off[i]:off[i + 1]])) for i in range(len(off) - 1)]
        row0 = len(self._vecs) if row0 is None else int(row0)
        assert 0 <= row0 <= len(self._vecs) and row0 + len(vectors) <= self.ntotal
        self.calls.append(("set_sparse", row0, len(vectors)))
        del self._vecs[row0:]
        for t, w in vectors:
            t, w = np.asarray(t, np.int64).reshape(-1), np.asarray(w, np.float32).reshape(-1)
            assert np.unique(t).size == t.size and (w > 0).all() and (t.size == 0 or (t.min() >= 0 and t.max() < TERM_SPACE))
            o = np.argsort(t)
            self._vecs.append((t[o], w[o]))

    def _sp(self, terms, weights):
        sp, hit = np.zeros(self.ntotal, np.float64), np.zeros(self.ntotal, bool)
        for r, (t, w) in enumerate(self._vecs):
            for q, qw in zip(terms, weights):
                at = np.flatnonzero(t == q)
                if at.size:
                    sp[r] += float(qw) * float(w[at[0]])
                    hit[r] = True
        return sp, hit

    @staticmethod
    def _query(terms, weights):
        terms = [int(t) for t in np.asarray(terms, np.int64).reshape(-1)]
        weights = np.asarray(weights, np.float32).reshape(-1)
        assert len(terms) == weights.shape[0] <= 64 and len(set(terms)) == len(terms) and (weights != 0).all()
        return terms, weights

    def search_sparse(self, terms, weights, k, allow=None):
        k = int(k)
        terms, weights = self._query(terms, weights)
        self.calls.append(("search_sparse", k, allow is not None, tuple(terms)))
        assert 1 <= k <= 128
        sp, hit = self._sp(terms, weights)
        ids = np.flatnonzero(self._ok(1, allow)[0] & hit)
        order = ids[np.lexsort((ids, -sp[ids]))][:k]
        D, I = np.full((1, k), -FLT_MAX, np.float32), np.full((1, k), -1, np.int64)
        D[0, :order.size], I[0, :order.size] = sp[order], order + self.base
        return D, I

    def search_hybrid_sparse(self, q, terms, weights, k, alpha, normalize=False, allow=None):
        k = int(k)
        terms, weights = self._query(terms, weights)
        self.calls.append(("search_hybrid_sparse", k, allow is not None, tuple(terms)))
        assert 1 <= k <= 128 and np.isfinite(alpha)
        q64 = np.asarray(q, np.float64).reshape(1, self.d)
        x64 = self._x.astype(np.float64)
        sp, _ = self._sp(terms, weights)
        if self.metric_type == 0:
            s = (q64 @ x64.T)[0]
            f = s + float(alpha) * sp
        else:
            s = ((q64 - x64) ** 2).sum(-1)
            f = s - float(alpha) * sp
        ids = np.flatnonzero(self._ok(1, allow)[0])
        order = ids[np.lexsort((ids, -f[ids] if self.metric_type == 0 else f[ids]))][:k]
        pad = -FLT_MAX if self.metric_type == 0 else FLT_MAX
        D, I = np.full((1, k), pad, np.float32), np.full((1, k), -1, np.int64)
        S, L = np.full((1, k), pad, np.float32), np.zeros((1, k), np.float32)
        D[0, :order.size], S[0, :order.size], L[0, :order.size], I[0, :order.size] = f[order], s[order], sp[order], order + self.base
        return D, I, S, L
