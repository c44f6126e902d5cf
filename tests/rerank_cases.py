"""The inputs and the float64 truth of the two-stage search tests (tests/test_rerank_maxsim_gpu.py), stated once, so that
tests/test_rerank_maxsim_host.py can prove with numpy alone that they make the exact checks of the GPU tests bind.
Nothing here touches a device and nothing here calls the code under test.

Dense rows are lattice rows (tests/lattice_cases.py, family T, searched with ``normalize=False``): every dense score is
an integer, exact on every search path, so the pool is ONE ``lexsort``.  The token matrices and the query matrices are
those of tests/tokens_cases.py (N = 3 001, six query lengths) and tests/tokens_codec_cases.py (N = 500): every late
score is exact in fp32 as well."""
import functools

import numpy as np

import lattice_cases as lc
import tokens_cases as tc
import tokens_codec_cases as cc
from tokens_fakes import Matrices

FMAX = np.finfo(np.float32).max
D = tc.D
FS = (1, 15, 16, 17, 50, 128)
NQS = (1, 2, 9, 1024)
KS = (1, 10, 128)


@functools.lru_cache(maxsize=4)
def dense(n, nq=16, seed=77):
    """(rows [n, D], queries [nq, D]) of family T."""
    x = lc.lattice_rows("T", n, D, seed)
    q = lc.lattice_queries("T", nq, D, seed + 1)
    x.setflags(write=False)
    q.setflags(write=False)
    return x, q


def batch(qs, nq):
    """nq query matrices: the six lengths in turn, so that equal queries stand at different positions; (pick, matrices)."""
    pick = np.arange(nq) % len(qs)
    return pick, [qs[i] for i in pick]


def decoded(codec, ms):
    """The matrices a compressed store scores: encode and decode in float64 (exact on the lattice inputs)."""
    codes, buckets = cc.encode64(codec, ms.tok)
    return Matrices(ms.off, cc.to_bits(cc.decode64(codec, codes, buckets).astype(np.float32)))


def id_lists(nq, f, n, T, seed, id_base=0):
    """ids [nq, f]: rows of [0, n) (repeats among them), with, where f allows, an empty row (row 0), a row >= T, and
    ids outside the index on both sides."""
    rng = np.random.default_rng(seed)
    ids = rng.integers(0, n, size=(nq, f)).astype(np.int64)
    if f >= 15:
        for b in range(nq):
            where = rng.permutation(f)[:5]
            ids[b, where] = (0, min(T, n - 1), -1, n, n + 7)
    return ids + id_base if id_base else ids


def lists64(ms, qs, ids, n, id_base=0):
    """float32 [nq, f] from float64 columns: the MaxSim of query b with row ids[b, j] - id_base; -inf for an id outside
    [0, n), a row beyond the matrices and an empty row.  (One column per DISTINCT query object.)"""
    full = ms.padded(n)
    cols = {}
    out = np.full(ids.shape, -np.inf)
    for b, q in enumerate(qs):
        col = cols.get(id(q))
        if col is None:
            col = cols[id(q)] = full.scores64(q)
        r = ids[b] - id_base
        ok = (r >= 0) & (r < n)
        out[b, ok] = col[r[ok]]
    assert np.array_equal(out.astype(np.float32).astype(np.float64), out)   # exact in fp32
    return out.astype(np.float32)


def rank(S0, I0, late, k, floor=None):
    """The oracle sentence of include/css_hip.h from the pool and its late scores: (D, I, S, R), each [nq, k]."""
    nq = S0.shape[0]
    D_, S = np.full((nq, k), -FMAX, np.float32), np.full((nq, k), -FMAX, np.float32)
    I, R = np.full((nq, k), -1, np.int64), np.full((nq, k), -1, np.int32)
    for b in range(nq):
        keep = [p for p in range(S0.shape[1]) if I0[b, p] >= 0 and late[b, p] > -np.inf
                and not (floor is not None and floor == floor and S0[b, p] < np.float32(floor))]
        keep.sort(key=lambda p: (-float(late[b, p]), p))
        for j, p in enumerate(keep[:k]):
            D_[b, j], I[b, j], S[b, j], R[b, j] = late[b, p], I0[b, p], S0[b, p], p
    return D_, I, S, R


def pool64(x, Q, fetch, metric=0, allow=None, id_base=0):
    """The dense pool (S0 float32 [nq, fetch], I0 int64) in float64 and one lexsort."""
    return lc.topk_of_scores(lc.scores64(x, Q, metric), fetch, metric, allow=allow, id_base=id_base)


def truth(x, Q, ms, qs, k, fetch, metric=0, floor=None, allow=None, id_base=0):
    """(D, I, S, R) of the two-stage search, and the pool and its late scores behind it."""
    S0, I0 = pool64(x, Q, fetch, metric, allow, id_base)
    late = lists64(ms, qs, I0, x.shape[0], id_base)
    return rank(S0, I0, late, k, floor), (S0, I0, late)


def tie_across(late_row, S0_row, I0_row, k, floor=None):
    """True when, among the entries of one pool that are ranked, the k-th and the (k + 1)-th late score are equal."""
    ok = (I0_row >= 0) & (late_row > -np.inf)
    if floor is not None:
        ok &= ~(S0_row < np.float32(floor))
    s = np.sort(-late_row[ok].astype(np.float64))
    return bool(s.shape[0] > k and s[k - 1] == s[k])
