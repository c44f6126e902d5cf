"""numpy TEST DOUBLE of the search by examples for the CPU tests of ``search_like`` and of the sharded
``search_examples``: ``related_fakes.FakeIndex`` plus ``search_examples``, stated INDEPENDENTLY of the library's way -- no
sweep, no lists, no merge: the scores of every row against every example, ``flat_index.fuse_example_scores`` (the
numpy statement of the fusion rule) and ONE ``lexsort`` by (value, id).  It lives in tests/ only; the product never
falls back to it.

Callers that compare a sharded with an unsharded double build rows, examples and gammas from multiples of 1/8, so that
every fused value is exact in float32."""
import numpy as np

from claude_semantic_search_amd.flat_index import fuse_example_scores
from related_fakes import FLT_MAX, FakeIndex


class FakeExamplesIndex(FakeIndex):
    def search_examples(self, pos=None, neg=None, pos_ids=(), neg_ids=(), k=10, gamma=0.5, normalize=False,
                        exclude_ids=True, allow=None):
        k = int(k)
        vec = lambda v: np.zeros((0, self.d), np.float32) if v is None or np.size(v) == 0 else np.asarray(v, np.float32).reshape(-1, self.d)  # noqa: E731
        ip = np.asarray(pos_ids, np.int64).reshape(-1) - self.base
        ineg = np.asarray(neg_ids, np.int64).reshape(-1) - self.base
        ids = np.concatenate([ip, ineg])
        assert ids.size == 0 or (ids.min() >= 0 and ids.max() < self.ntotal)
        ep = np.concatenate([vec(pos), self._x[ip]])
        en = np.concatenate([vec(neg), self._x[ineg]])
        assert 1 <= k <= 128 and np.isfinite(gamma) and gamma >= 0 and ep.shape[0] >= 1 and ep.shape[0] + en.shape[0] <= 16
        self.calls.append(("search_examples", k, allow is not None, ep.shape[0], en.shape[0], bool(exclude_ids)))
        pad = -FLT_MAX if self.metric_type == 0 else FLT_MAX
        D, I, S = np.full(k, pad, np.float32), np.full(k, -1, np.int64), np.full(k, pad, np.float32)
        if self.ntotal == 0:
            return D, I, S
        F, P = fuse_example_scores(self._scores(ep), self._scores(en) if en.shape[0] else np.zeros((0, self.ntotal), np.float32),
                                   gamma, self.metric_type)
        ok = self._ok(1, allow)[0]
        if exclude_ids:
            ok[ids] = False
        rows = np.flatnonzero(ok)
        order = rows[np.lexsort((rows, -F[rows] if self.metric_type == 0 else F[rows]))][:k]
        D[:order.size], S[:order.size], I[:order.size] = F[order], P[order], order + self.base
        return D, I, S
