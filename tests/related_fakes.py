"""numpy TEST DOUBLE of the device index for the CPU tests of ``search_by_ids`` / ``search_related``: the contract of
``IndexFlat`` (scores best first, ties to the lower id, ``-1`` / ``-+FLT_MAX`` padding, allow masks, ``id_base``) with
``search_by_ids`` stated INDEPENDENTLY of the library's way (no ``k + 1`` search and no drop: the anchor's row is simply
taken out of the candidates).  It lives in tests/ only; the product never falls back to it.

Callers build rows from multiples of 1/8 so that every score is exact in float32 whatever the summation order: a
sharded and an unsharded double then give the same bits, and ties are plentiful."""
import numpy as np

FLT_MAX = np.finfo(np.float32).max


class FakeIndex:
    def __init__(self, d, metric=0, device=0):
        self.d, self.metric_type, self.device, self.base = int(d), int(metric), device, 0
        self._x = np.zeros((0, self.d), np.float32)
        self.calls = []   # (method, k, allow is not None), newest last

    ntotal = property(lambda self: self._x.shape[0])

    def add(self, x, normalize=False):   # (`normalize` is the device's business, tested on the GPU: rows stay as given)
        self._x = np.concatenate([self._x, np.asarray(x, np.float32).reshape(-1, self.d)])

    def set_id_base(self, b):
        self.base = int(b)

    def reserve(self, n):
        pass

    def close(self):
        pass

    def reconstruct_n(self, row0=0, n=None):
        n = self.ntotal - row0 if n is None else n
        return self._x[row0:row0 + n].copy()

    def _scores(self, q):
        x64, q64 = self._x.astype(np.float64), np.asarray(q, np.float64).reshape(-1, self.d)
        if self.metric_type == 0:
            return (q64[:, None, :] * x64[None, :, :]).sum(-1).astype(np.float32)
        return ((q64[:, None, :] - x64[None, :, :]) ** 2).sum(-1).astype(np.float32)

    def _topk(self, s, ok, k):
        """s, ok: [nq, ntotal] scores and candidate flags -> padded (D, I) with global ids."""
        nq = s.shape[0]
        D = np.full((nq, k), -FLT_MAX if self.metric_type == 0 else FLT_MAX, np.float32)
        I = np.full((nq, k), -1, np.int64)
        for j in range(nq):
            ids = np.flatnonzero(ok[j])
            order = np.lexsort((ids, -s[j, ids] if self.metric_type == 0 else s[j, ids]))[:k]
            D[j, :order.size] = s[j, ids][order]
            I[j, :order.size] = ids[order] + self.base
        return D, I

    def _ok(self, nq, allow):
        ok = np.ones((nq, self.ntotal), bool)
        if allow is not None:
            a = np.asarray(allow)
            assert a.dtype == np.bool_ and a.shape == (self.ntotal,)
            ok &= a[None, :]
        return ok

    def search(self, q, k, normalize=False, allow=None):
        self.calls.append(("search", int(k), allow is not None))
        s = self._scores(q)
        return self._topk(s, self._ok(s.shape[0], allow), int(k))

    def search_by_ids(self, ids, k, exclude_self=True, allow=None):
        self.calls.append(("search_by_ids", int(k), allow is not None))
        a = np.asarray(ids, np.int64).reshape(-1) - self.base
        assert a.size == 0 or (a.min() >= 0 and a.max() < self.ntotal)
        s = self._scores(self._x[a]) if a.size else np.zeros((0, self.ntotal), np.float32)
        ok = self._ok(a.size, allow)
        if exclude_self:
            ok[np.arange(a.size), a] = False
        return self._topk(s, ok, int(k))


def merge_lists(metric):
    """``merge=`` of ``ShardedFlatIndex`` for CPU tensors: [world, nq, k] lists -> top-k by (score, id), pads last."""
    import torch

    def f(Dg, Ig, k):
        D, I = Dg.numpy(), Ig.numpy()
        w, nq, kk = D.shape
        Dm, Im = np.empty((nq, k), np.float32), np.empty((nq, k), np.int64)
        for j in range(nq):
            d, i = D[:, j].reshape(-1), I[:, j].reshape(-1)
            order = np.lexsort((i, -d if metric == 0 else d, i < 0))[:k]
            Dm[j], Im[j] = d[order], i[order]
        return torch.from_numpy(Dm), torch.from_numpy(Im)
    return f
