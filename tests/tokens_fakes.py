"""numpy statements of the token-matrix side of the flat index for the tests; they live in tests/ only and the product
never falls back to them.

* ``Matrices`` -- CSR token matrices (uint16 bf16 bits).  ``scores64`` is the MaxSim of ONE query against every row in
  float64 from the bf16 values (widened exactly): one matmul, the per-row maximum by ``np.maximum.reduceat``, the sum
  over the query's tokens; ``-inf`` for a row without tokens.  tests/test_tokens_index_host.py checks it against
  ``late_interaction.maxsim_numpy`` row by row.
* ``topk`` -- the ranking of the search: rows that are no miss and are allowed, by ONE ``lexsort`` on (score
  descending, id ascending).
* ``FakeTokenIndex`` -- ``prior_fakes.FakePriorIndex`` plus token matrices: the TEST DOUBLE of the device index for the
  CPU tests of the sharded ``search_maxsim`` / ``maxsim_ids``.  Every value in fp64 and ONE ``lexsort``."""
import numpy as np

from claude_semantic_search_amd.late_interaction import bf16_to_f32
from prior_fakes import FakePriorIndex
from related_fakes import FLT_MAX


class Matrices:
    def __init__(self, off, tok):
        self.off = np.ascontiguousarray(off, np.int64)
        self.tok = np.ascontiguousarray(tok, np.uint16)
        assert self.tok.ndim == 2 and self.off[0] == 0 and self.off[-1] == self.tok.shape[0]
        self.n, self.P = self.off.shape[0] - 1, self.tok.shape[1]

    @classmethod
    def of(cls, mats, P):
        """From a list of [m_i, P] uint16 matrices."""
        off = np.concatenate([[0], np.cumsum([m.shape[0] for m in mats])]).astype(np.int64)
        return cls(off, np.concatenate(mats) if mats else np.zeros((0, P), np.uint16))

    @property
    def lens(self):
        return np.diff(self.off)

    def mat(self, r):
        return self.tok[self.off[r]:self.off[r + 1]]

    def mats(self):
        return [self.mat(r) for r in range(self.n)]

    @property
    def csr(self):
        return self.off, self.tok, self.P

    def scores64(self, q):
        """float64 [n]: sum_s max_t dot(q_s, d_t) per row, -inf for a row without tokens."""
        q64 = bf16_to_f32(q).astype(np.float64)
        out = np.full(self.n, -np.inf)
        live = np.flatnonzero(self.lens > 0)
        if live.size:
            sim = q64 @ bf16_to_f32(self.tok).astype(np.float64).T           # [mq, E]
            out[live] = np.maximum.reduceat(sim, self.off[:-1][live], axis=1).sum(axis=0)
        return out

    def rows(self, sel):
        """The matrices of the selected rows (a boolean mask or row numbers), in that order, as a new ``Matrices``."""
        sel = np.flatnonzero(sel) if np.asarray(sel).dtype == np.bool_ else np.asarray(sel, np.int64)
        return Matrices.of([self.mat(int(r)) for r in sel], self.P)

    def padded(self, n):
        """The same matrices on an index of n >= self.n rows: the rows behind them have none."""
        return Matrices(np.concatenate([self.off, np.full(n - self.n, self.off[-1])]), self.tok)


def topk(scores, k, allowed=None, id_base=0):
    """(D float32 [1, k], I int64 [1, k]) of the MaxSim search from a float64 column with -inf for the misses."""
    ok = scores > -np.inf
    if allowed is not None:
        ok = ok & np.asarray(allowed, bool)
    ids = np.flatnonzero(ok)
    order = ids[np.lexsort((ids, -scores[ids]))][:k]
    D, I = np.full((1, k), -FLT_MAX, np.float32), np.full((1, k), -1, np.int64)
    D[0, :order.size], I[0, :order.size] = scores[order], order + id_base
    return D, I


def ties_at(scores, k, allowed=None):
    """True when the k-th and the (k+1)-th best allowed hit of the column have the same score."""
    ok = scores > -np.inf
    if allowed is not None:
        ok = ok & np.asarray(allowed, bool)
    s = np.sort(-scores[ok])
    return bool(s.shape[0] > k and s[k - 1] == s[k])


class FakeTokenIndex(FakePriorIndex):
    def __init__(self, d, metric=0, device=0):
        super().__init__(d, metric, device)
        self._mats = []   # per leading row: uint16 [m, P]
        self._P = 0

    @property
    def token_rows(self):
        return len(self._mats)

    @property
    def token_dim(self):
        return self._P if self._mats else 0

    def drop_tokens(self):
        self._mats, self._P = [], 0

    def set_tokens(self, mats, keep=None, row0=None):
        from claude_semantic_search_amd.flat_index import tokens_as_csr

        off, tok, P = tokens_as_csr(mats, keep)
        row0 = len(self._mats) if row0 is None else int(row0)
        n = off.shape[0] - 1
        assert 0 <= row0 <= len(self._mats) and row0 + n <= self.ntotal
        assert not self._mats or row0 == 0 or n == 0 or P == self._P
        self.calls.append(("set_tokens", row0, n))
        if n == 0 and row0 == len(self._mats):
            return
        del self._mats[row0:]
        self._mats += [tok[off[i]:off[i + 1]].copy() for i in range(n)]
        self._P = P if n else self._P

    def get_tokens(self, row0=0, n=None):
        n = self.ntotal - row0 if n is None else n
        P = self.token_dim
        mats = [self._mats[r] if r < len(self._mats) else np.zeros((0, P), np.uint16) for r in range(row0, row0 + n)]
        m = Matrices.of(mats, P)
        return m.off, m.tok

    def _column(self, q):
        q = np.asarray(q, np.uint16)
        assert q.ndim == 2 and 1 <= q.shape[0] <= 64 and (not self._mats or q.shape[1] == self._P)
        if not self._mats:
            return np.full(self.ntotal, -np.inf)
        return Matrices.of(self._mats, self._P).padded(self.ntotal).scores64(q)

    def search_maxsim(self, q_mat, k, allow=None):
        k = int(k)
        self.calls.append(("search_maxsim", k, allow is not None))
        assert 1 <= k <= 128
        return topk(self._column(q_mat), k, self._ok(1, allow)[0], self.base)

    def maxsim_ids(self, q_mat, ids):
        a = np.asarray(ids, np.int64).reshape(-1) - self.base
        assert ((a >= 0) & (a < self.ntotal)).all()
        self.calls.append(("maxsim_ids", a.shape[0]))
        return self._column(q_mat)[a].astype(np.float32)
