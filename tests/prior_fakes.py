"""numpy TEST DOUBLE of the prior-weighted search for the CPU tests of ``search_recent`` and of the sharded
``search_prior``: ``related_fakes.FakeIndex`` plus the prior column.  ``search_prior`` is stated INDEPENDENTLY of the
library's way -- no sweep, no lists, no merge: the fused value of every allowed row in fp64 and ONE ``lexsort`` by
(value, id).  It lives in tests/ only; the product never falls back to it.

Callers that compare a sharded with an unsharded double build rows, priors and weights from multiples of 1/8, so that
every fused value is exact in float32."""
import numpy as np

from related_fakes import FLT_MAX, FakeIndex


class FakePriorIndex(FakeIndex):
    def __init__(self, d, metric=0, device=0):
        super().__init__(d, metric, device)
        self._p = np.zeros(0, np.float32)

    def add(self, x, normalize=False):
        super().add(x, normalize)
        self._p = np.concatenate([self._p, np.zeros(self.ntotal - self._p.shape[0], np.float32)])

    def set_priors(self, priors, row0=0):
        a = np.asarray(priors)
        assert a.ndim == 1 and a.dtype != np.bool_ and np.issubdtype(a.dtype, np.number)
        assert 0 <= row0 and row0 + a.shape[0] <= self.ntotal and np.isfinite(a).all()
        self.calls.append(("set_priors", int(row0), int(a.shape[0])))
        self._p[row0:row0 + a.shape[0]] = a.astype(np.float32)

    def get_priors(self, row0=0, n=None):
        n = self.ntotal - row0 if n is None else n
        return self._p[row0:row0 + n].copy()

    def search_prior(self, q, k, weight, normalize=False, allow=None):
        self.calls.append(("search_prior", int(k), allow is not None))
        k = int(k)
        assert 1 <= k <= 128 and np.isfinite(weight)
        q64 = np.asarray(q, np.float64).reshape(-1, self.d)
        x64 = self._x.astype(np.float64)
        nq = q64.shape[0]
        wp = np.float64(np.float32(weight)) * self._p.astype(np.float64)
        if self.metric_type == 0:
            s = q64 @ x64.T
            f = s + wp[None, :]
        else:
            s = ((q64[:, None, :] - x64[None, :, :]) ** 2).sum(-1)
            f = s - wp[None, :]
        ok = self._ok(nq, allow)
        pad = -FLT_MAX if self.metric_type == 0 else FLT_MAX
        D, I, S = np.full((nq, k), pad, np.float32), np.full((nq, k), -1, np.int64), np.full((nq, k), pad, np.float32)
        for j in range(nq):
            ids = np.flatnonzero(ok[j])
            order = ids[np.lexsort((ids, -f[j, ids] if self.metric_type == 0 else f[j, ids]))][:k]
            D[j, :order.size], S[j, :order.size], I[j, :order.size] = f[j, order], s[j, order], order + self.base
        return D, I, S
