"""The numpy double of the two-stage search for the CPU tests: ``tokens_batch_fakes.FakeTokenBatchIndex`` plus
``maxsim_ids_batch`` and ``search_rerank_maxsim``, composed from the double's own ``search`` and float64 columns by the
oracle sentence of include/css_hip.h.  It lives in tests/ only."""
import numpy as np

from claude_semantic_search_amd import flat_index as fi
from tokens_batch_fakes import FakeTokenBatchIndex


class FakeRerankIndex(FakeTokenBatchIndex):
    def maxsim_ids_batch(self, q_mats, ids):
        _, off, tok, _, f, _, ids = fi.rerank_args(None, q_mats, None, None, ids=ids, what="maxsim_ids_batch")
        nq = off.shape[0] - 1
        self.calls.append(("maxsim_ids_batch", nq, f))
        out = np.full((nq, f), -np.inf, np.float32)
        for b in range(nq):
            r = ids[b] - self.base
            ok = (r >= 0) & (r < self.ntotal)
            out[b, ok] = self._column(tok[off[b]:off[b + 1]])[r[ok]]
        return out

    def search_rerank_maxsim(self, q, q_mats, k, fetch, normalize=False, floor=None, allow=None):
        a, off, tok, k, fetch, floor, _ = fi.rerank_args(q, q_mats, k, fetch, floor, d=self.d)
        nq = off.shape[0] - 1
        self.calls.append(("search_rerank_maxsim", nq, k, fetch, allow is not None))
        S0, I0 = self.search(a, fetch, normalize=normalize, allow=allow)
        late = self.maxsim_ids_batch([tok[off[b]:off[b + 1]] for b in range(nq)], I0)
        return fi.search_rerank_maxsim_numpy(S0, I0, late, k, floor)
