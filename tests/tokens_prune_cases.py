"""The inputs of tests/test_tokens_prune_gpu.py, stated once, so that tests/test_tokens_prune_host.py can prove with numpy
alone that they make the exact checks of the GPU tests bind.  Nothing here touches a device.

The lattice cases are those of tests/tokens_codec_cases.py (``lattice(P, nbits, C)``): every centroid dot S, every
approximate score A and every exact score is a sum of multiples of 1/64 far below 2^24 units, exact in fp32 in any
order, and docs drawn from one pool tie.  The wide case exists for the select alone: 40 077 rows of 0 to 3 lattice
tokens from a pool of about 200 distinct docs, so thousands of rows tie on A, across the 4096-row slices of the
compaction."""
import functools

import numpy as np

import tokens_codec_cases as cc
from claude_semantic_search_amd import flat_index as fi
from tokens_fakes import Matrices

N = cc.N
NCANDS = (16, 100, 499, 500, 65536)          # and k itself, per test
KS = (1, 10, 128)
SLICE = 4096                                 # rows of one block of the select's compaction (kSelSlice)

WIDE_N = 40077
WIDE_P, WIDE_C, WIDE_BITS = 32, 17, 2
WIDE_POOL = 200
WIDE_NCANDS = (1, 128, 4097, 40077, 65536)


@functools.lru_cache(maxsize=64)
def lattice_codes(P, nbits, C):
    """(codec, Matrices, queries, codes, res) of a lattice case: the codes of the numpy double."""
    codec, ms, qs = cc.lattice(P, nbits, C)
    codes, res = fi.token_codec_encode(codec, ms.tok)
    return codec, ms, qs, codes, res


@functools.lru_cache(maxsize=1)
def wide():
    """(codec, Matrices over WIDE_N rows, query uint16 [17, P], codes, res)."""
    P, C = WIDE_P, WIDE_C
    codec = cc.lattice_codec(P, WIDE_BITS, C, seed=5)
    rng = np.random.default_rng(4242)
    lens = rng.integers(0, 4, size=WIDE_POOL)
    lens[:4] = (0, 1, 2, 3)
    pool = []
    for m in lens:
        base = codec.centroids[rng.integers(0, C, size=m)]
        pool.append(cc.to_bits(np.clip(base + rng.integers(-1, 2, size=(m, P)) / 8.0, -1.0, 1.0).astype(np.float32)))
    pick = rng.integers(0, WIDE_POOL, size=WIDE_N)
    off = np.concatenate([[0], np.cumsum(lens[pick])]).astype(np.int64)
    tok = np.concatenate([pool[i] for i in pick])
    ms = Matrices(off, tok)
    q = cc.to_bits((rng.integers(-8, 9, size=(17, P)) / 8.0).astype(np.float32))
    codes, res = fi.token_codec_encode(codec, ms.tok)
    return codec, ms, q, codes, res


def approx64(codec, off, codes, q):
    """The float64 restatement of the approximate score: float64 [n], -inf for a row without tokens."""
    S = codec.centroids.astype(np.float64) @ fi.bf16_to_f32(q).astype(np.float64).T        # [C, mq]
    off = np.asarray(off, np.int64)
    out = np.full(off.shape[0] - 1, -np.inf)
    live = np.flatnonzero(np.diff(off) > 0)
    if live.size:
        out[live] = np.maximum.reduceat(S[codes], off[:-1][live], axis=0).sum(axis=1)
    return out


def candidates64(a64, ncand, allowed=None):
    """Rows (ascending) of the first ncand of lexsort((row, -A)) among the allowed rows that are no miss."""
    ok = a64 > -np.inf
    if allowed is not None:
        ok = ok & np.asarray(allowed, bool)
    rows = np.flatnonzero(ok)
    return np.sort(rows[np.lexsort((rows, -a64[rows]))][:ncand])


def exact64(codec, ms, codes, res, q):
    """float64 exact scores on the codes: those of the decoded matrices."""
    return Matrices(ms.off, fi.token_codec_decode(codec, codes, res)).scores64(q)


def pruned64(a64, e64, k, ncand, allowed=None, id_base=0):
    """(D float32 [1, k], I int64 [1, k]) of the pruned search from the float64 columns."""
    rows = candidates64(a64, ncand, allowed)
    order = rows[np.lexsort((rows, -e64[rows]))][:k]
    D, I = np.full((1, k), -np.finfo(np.float32).max, np.float32), np.full((1, k), -1, np.int64)
    D[0, :order.size], I[0, :order.size] = e64[order], order + id_base
    return D, I


def ties_across(a64, ncand, allowed=None):
    """True when the rows at ranks ncand and ncand + 1 of the approximate ranking have the same A."""
    ok = a64 > -np.inf
    if allowed is not None:
        ok = ok & np.asarray(allowed, bool)
    s = np.sort(-a64[ok])
    return bool(s.shape[0] > ncand and s[ncand - 1] == s[ncand])
