"""The numpy double of the batched MaxSim search for the CPU tests: ``tokens_fakes.FakeTokenIndex`` plus
``search_maxsim_batch``, which is the loop of single calls by definition.  It lives in tests/ only."""
import numpy as np

from claude_semantic_search_amd import flat_index as fi
from tokens_fakes import FakeTokenIndex


class FakeTokenBatchIndex(FakeTokenIndex):
    last_maxsim_passes = 0

    def search_maxsim_batch(self, q_mats, k, allow=None):
        off, tok, k = fi.maxsim_batch_args(q_mats, k)
        nq = off.shape[0] - 1
        self.calls.append(("search_maxsim_batch", nq, k, allow is not None))
        rows = [self.search_maxsim(tok[off[b]:off[b + 1]], k, allow=allow) for b in range(nq)]
        scanned = bool(self._mats) and self.ntotal > 0
        self.last_maxsim_passes = -(-nq // fi.MAXSIM_BATCH_GROUP) if scanned else 0
        return np.concatenate([r[0] for r in rows]), np.concatenate([r[1] for r in rows])
