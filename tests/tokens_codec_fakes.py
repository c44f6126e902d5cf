"""``FakeCodecIndex`` -- ``tokens_fakes.FakeTokenIndex`` plus a token codec: the TEST DOUBLE of the device index for the
CPU tests of the sharded compressed token matrices.  With a codec it keeps, per row, the canonical codes of the numpy
double (``flat_index.token_codec_encode``) and scores the decoded matrices (``token_codec_decode``) in fp64 with ONE
``lexsort``; without one it is ``FakeTokenIndex``.  It lives in tests/ only and the product never falls back to it."""
import numpy as np

from claude_semantic_search_amd import flat_index as fi
from tokens_fakes import FakeTokenIndex


class FakeCodecIndex(FakeTokenIndex):
    def __init__(self, d, metric=0, device=0):
        super().__init__(d, metric, device)
        self._codec = None
        self._codes = []   # per leading row: (codes uint16 [m], res uint8 [m, RB])

    @property
    def token_codec_bits(self):
        return 0 if self._codec is None else self._codec.nbits

    def get_token_codec(self):
        return self._codec

    def set_token_codec(self, codec):
        assert self.token_rows == 0, "the codec changes only while there are no matrices"
        self._codec = None if codec is None else fi.token_codec_args(*codec)
        self.calls.append(("set_token_codec", self.token_codec_bits))

    def drop_tokens(self):
        super().drop_tokens()
        self._codes = []

    def _store(self, row0, off, codes, res):
        """Rows [row0, row0 + n) from canonical codes: the decoded matrices are what the searches see."""
        n = off.shape[0] - 1
        assert 0 <= row0 <= len(self._mats) and row0 + n <= self.ntotal
        if n == 0 and row0 == len(self._mats):
            return
        dec = fi.token_codec_decode(self._codec, codes, res)
        del self._mats[row0:], self._codes[row0:]
        self._mats += [dec[off[i]:off[i + 1]].copy() for i in range(n)]
        self._codes += [(codes[off[i]:off[i + 1]].copy(), res[off[i]:off[i + 1]].copy()) for i in range(n)]
        self._P = self._codec.P if n else self._P

    def set_tokens(self, mats, keep=None, row0=None):
        if self._codec is None:
            return super().set_tokens(mats, keep=keep, row0=row0)
        off, tok, P = fi.tokens_as_csr(mats, keep)
        assert off.shape[0] == 1 or P == self._codec.P
        row0 = len(self._mats) if row0 is None else int(row0)
        self.calls.append(("set_tokens", row0, off.shape[0] - 1))
        self._store(row0, off, *fi.token_codec_encode(self._codec, tok.reshape(-1, self._codec.P)))

    def set_token_codes(self, offsets, codes, res, row0=None):
        off, codes, res = fi.token_codes_as_csr(offsets, codes, res, self._codec)
        row0 = len(self._mats) if row0 is None else int(row0)
        self.calls.append(("set_token_codes", row0, off.shape[0] - 1))
        self._store(row0, off, codes, res)

    def get_token_codes(self, row0=0, n=None):
        n = self.ntotal - row0 if n is None else n
        RB = self._codec.res_bytes
        rows = [self._codes[r] if r < len(self._codes) else (np.zeros(0, np.uint16), np.zeros((0, RB), np.uint8))
                for r in range(row0, row0 + n)]
        off = np.concatenate([[0], np.cumsum([c.shape[0] for c, _ in rows])]).astype(np.int64)
        codes = np.concatenate([c for c, _ in rows]) if rows else np.zeros(0, np.uint16)
        res = np.concatenate([r for _, r in rows]) if rows else np.zeros((0, RB), np.uint8)
        return off, codes.astype(np.uint16), res.reshape(-1, RB).astype(np.uint8)
