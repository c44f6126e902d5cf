"""numpy TEST DOUBLE of the grouped search for the CPU tests of ``search_sessions`` and of the sharded grouped search:
``related_fakes.FakeIndex`` plus the label column.  ``search_grouped`` is stated INDEPENDENTLY of the library's way -- no
ranked list, no passes, no collapse: every group's best allowed row is found as a per-group maximum under the total
order (score, then lower id), every ungrouped allowed row stands for itself, and the representatives are ranked.  It
lives in tests/ only; the product never falls back to it."""
import numpy as np

from related_fakes import FLT_MAX, FakeIndex


class FakeGroupedIndex(FakeIndex):
    def __init__(self, d, metric=0, device=0):
        super().__init__(d, metric, device)
        self._g = np.zeros(0, np.int32)

    def add(self, x, normalize=False):
        super().add(x, normalize)
        self._g = np.concatenate([self._g, np.full(self.ntotal - self._g.shape[0], -1, np.int32)])

    def set_groups(self, labels, row0=0):
        a = np.asarray(labels)
        assert np.issubdtype(a.dtype, np.integer) and a.ndim == 1 and 0 <= row0 and row0 + a.shape[0] <= self.ntotal
        self.calls.append(("set_groups", int(row0), int(a.shape[0])))
        self._g[row0:row0 + a.shape[0]] = np.maximum(a, -1)

    def get_groups(self, row0=0, n=None):
        n = self.ntotal - row0 if n is None else n
        return self._g[row0:row0 + n].copy()

    def search_grouped(self, q, k, normalize=False, allow=None):
        self.calls.append(("search_grouped", int(k), allow is not None))
        s = self._scores(q)
        nq, k = s.shape[0], int(k)
        ok = self._ok(nq, allow)
        D = np.full((nq, k), -FLT_MAX if self.metric_type == 0 else FLT_MAX, np.float32)
        I = np.full((nq, k), -1, np.int64)
        G = np.full((nq, k), -1, np.int32)
        for j in range(nq):
            key = -s[j] if self.metric_type == 0 else s[j]            # smaller = better
            reps = [int(r) for r in np.flatnonzero(ok[j] & (self._g < 0))]
            for g in np.unique(self._g[ok[j] & (self._g >= 0)]):
                rows = np.flatnonzero(ok[j] & (self._g == g))
                reps.append(int(rows[np.flatnonzero(key[rows] == key[rows].min())[0]]))   # per-group maximum, lowest id
            reps.sort(key=lambda r: (key[r], r))
            for m, r in enumerate(reps[:k]):
                D[j, m], I[j, m], G[j, m] = s[j, r], r + self.base, self._g[r]
        return D, I, G
