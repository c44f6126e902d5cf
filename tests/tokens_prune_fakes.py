"""``FakePruneIndex`` -- ``tokens_codec_fakes.FakeCodecIndex`` plus the candidate stage: the TEST DOUBLE of the device
index for the CPU tests of the sharded ``maxsim_candidates`` / ``search_maxsim_pruned``.  The approximate column is the
float64 MaxSim of ``centroids[codes]``, the exact one that of the decoded matrices, and every ranking is ONE
``lexsort``.  It lives in tests/ only and the product never falls back to it."""
import numpy as np

from related_fakes import FLT_MAX
from tokens_codec_fakes import FakeCodecIndex
from tokens_fakes import Matrices


class FakePruneIndex(FakeCodecIndex):
    def _approx(self, q):
        q = np.asarray(q, np.uint16)
        assert self._codec is not None, "the index has no token codec"
        if not self._codes:
            return np.full(self.ntotal, -np.inf)
        cent = (self._codec.centroids.view(np.uint32) >> 16).astype(np.uint16)
        mats = [cent[c] for c, _ in self._codes]
        return Matrices.of(mats, self._codec.P).padded(self.ntotal).scores64(q)

    def _candidates(self, q, ncand, allow):
        a = self._approx(q)
        ok = (a > -np.inf) & self._ok(1, allow)[0]
        rows = np.flatnonzero(ok)
        return np.sort(rows[np.lexsort((rows, -a[rows]))][:ncand]), a

    def maxsim_candidates(self, q_mat, ncand, allow=None):
        ncand = int(ncand)
        assert 1 <= ncand <= 65536
        self.calls.append(("maxsim_candidates", ncand, allow is not None))
        rows, a = self._candidates(q_mat, ncand, allow)
        return rows.astype(np.int64) + self.base, a[rows].astype(np.float32)

    def search_maxsim_pruned(self, q_mat, k, ncand, allow=None):
        k, ncand = int(k), int(ncand)
        assert 1 <= k <= 128 and k <= ncand <= 65536
        self.calls.append(("search_maxsim_pruned", k, ncand, allow is not None))
        rows, _ = self._candidates(q_mat, ncand, allow)
        col = self._column(q_mat)
        order = rows[np.lexsort((rows, -col[rows]))][:k]
        D, I = np.full((1, k), -FLT_MAX, np.float32), np.full((1, k), -1, np.int64)
        D[0, :order.size], I[0, :order.size] = col[order], order + self.base
        return D, I
