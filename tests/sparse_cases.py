"""The inputs of tests/test_sparse_index_gpu.py, stated once, so that tests/test_sparse_index_host.py can prove with
numpy alone that they make every check of the GPU tests bind.  Nothing here touches a device."""
import functools

import numpy as np

from claude_semantic_search_amd import synth
from sparse_fakes import Vectors, topk_slice

N = 20003                    # not a multiple of 64 or 256: the last wave and block are partial
VOCAB = 4096
KS = (1, 10, 128)
MS = (1, 4, 32, 33, 64)      # 32 | 33: the two instantiations of k_sparse_scores
ID_BASE = 10 ** 9
HYBRID_ALPHA = 0.5
HYBRID_MS = (1, 4, 8, 16, 32, 33, 48, 64)   # the term-set sizes of the 8 (query, term set) pairs of the hybrid grid


@functools.lru_cache(maxsize=4)
def vectors(seed, lattice=False):
    return Vectors(*synth.sparse_vectors(N, seed, VOCAB, lattice=lattice))


def query(j, m, lattice=False, signed=False):
    """Query j: m distinct terms with the u^3 skew of the vectors, in order of first occurrence, and their weights:
    log1p of an exponential draw, or multiples of 1/8 in (0, 4] (lattice); signed: every third weight negated."""
    rng = np.random.default_rng(700 + j)
    t = np.floor(VOCAB * rng.random(64 * m + 64) ** 3).astype(np.int64)
    t = t[np.sort(np.unique(t, return_index=True)[1])][:m]
    assert t.shape[0] == m
    if lattice:
        w = (rng.integers(1, 33, size=m) / 8.0).astype(np.float32)
    else:
        w = np.maximum(np.log1p(rng.standard_exponential(m)).astype(np.float32), np.float32(2.0 ** -20))
    if signed:
        w[2::3] *= np.float32(-1.0)
    return t, w


def half_mask():
    return np.random.default_rng(6).random(N) < 0.5


def pure_queries(vs, lattice=False):
    """name -> (terms, weights) of the pure search cases over the vectors `vs`: one query per m of MS, a signed one, the
    rarest stored term alone (fewer than 10 hits) and two terms that no row stores (no hit at all)."""
    out = {f"m={m}": query(m, m, lattice) for m in MS}
    out["signed m=8"] = query(8, 8, lattice, signed=True)
    stored, df = np.unique(vs.terms, return_counts=True)
    out["rarest term"] = (np.array([int(stored[np.argmin(df)])], np.int64), np.array([1.5], np.float32))
    out["no such term"] = (np.array([VOCAB + 904, VOCAB + 1904], np.int64), np.array([1.0, 2.0], np.float32))
    return out


def slices():
    """The first row of every block of the column top-k over N rows."""
    return np.arange(0, N, topk_slice(N))


# ---------------------------------------------------------------------------------------------------------------------
# the list shapes at which k_sparse_scores takes another path
SHAPES_T = 12000             # rows [SHAPES_T, N) have no vector
LONG_ROW, MAXTERM_ROW, ALL64_ROW, CHAIN_ROW, CANCEL_ROW = 2500, 2502, 2503, 2504, 2505
CHAIN = (100, 4196, 8292)    # equal low 12 bits: three in one chain of the slot table
MAXTERM = (1 << 24) - 1


@functools.lru_cache(maxsize=1)
def shapes():
    """(Vectors over N rows, {name: (terms, weights)})."""
    rng = np.random.default_rng(43)
    base = vectors(201).rows(np.arange(SHAPES_T))
    rows = [(base.terms[base.off[r]:base.off[r + 1]].astype(np.int64), base.w[base.off[r]:base.off[r + 1]]) for r in range(SHAPES_T)]
    empty = (np.zeros(0, np.int64), np.zeros(0, np.float32))
    for r in rng.choice(SHAPES_T, size=300, replace=False):
        rows[int(r)] = empty                                                    # scattered empty rows
    for r in range(1024, 1216):
        rows[r] = empty                                                         # waves whose 64 rows are all empty
    rows[0] = empty
    all64_t, all64_w = query(64, 64)
    long_t = np.concatenate([all64_t[:32], 5000 + rng.choice(1 << 20, size=1968, replace=False)])
    rows[LONG_ROW] = (rng.permutation(long_t), (0.25 + rng.random(2000)).astype(np.float32))   # 2 000 entries, any order
    rows[MAXTERM_ROW] = (np.array([MAXTERM, 3], np.int64), np.array([2.0, 0.5], np.float32))
    rows[ALL64_ROW] = (all64_t[::-1].copy(), (0.5 + rng.random(64)).astype(np.float32))       # all 64 query terms
    rows[CHAIN_ROW] = (np.array([8292, 100, 4196, 20580], np.int64), np.array([0.75, 0.5, 1.25, 3.0], np.float32))
    rows[CANCEL_ROW] = (np.array([VOCAB + 7, VOCAB + 9], np.int64), np.array([1.5, 1.5], np.float32))
    rows[CANCEL_ROW + 1] = (np.array([VOCAB + 21], np.int64), np.array([1.0], np.float32))            # a positive row
    rows[CANCEL_ROW + 2] = (np.array([VOCAB + 21, 5], np.int64), np.array([2.0, 1.0], np.float32))    # another
    rows[CANCEL_ROW + 3] = (np.array([VOCAB + 23], np.int64), np.array([1.0], np.float32))            # a negative row
    rows[SHAPES_T - 1] = (np.array([5, 9], np.int64), np.array([1.0, 2.0], np.float32))
    off = np.concatenate([[0], np.cumsum([t.shape[0] for t, _ in rows])])
    vs = Vectors(off, np.concatenate([t for t, _ in rows]), np.concatenate([w for _, w in rows])).padded(N)
    queries = {
        "64 terms, one row holds them all": (all64_t, all64_w),
        "the same reversed": (all64_t[::-1].copy(), all64_w[::-1].copy()),
        "32 terms of the long row": (all64_t[:32], all64_w[:32]),
        "largest term id": (np.array([MAXTERM, 3], np.int64), np.array([0.5, 0.25], np.float32)),
        "shared low bits": (np.array([8292, 100, 12388, 20580, 4196], np.int64), np.array([0.11, 0.07, 0.5, 0.03, 0.05], np.float32)),
        "no term occurs": (np.array([VOCAB + 11, 12388], np.int64), np.array([1.0, 1.0], np.float32)),
        # 1.5 x 0.5 and 1.5 x -0.5 cancel on CANCEL_ROW; the next two rows are positive, the third negative
        "cancellation": (np.array([VOCAB + 7, VOCAB + 9, VOCAB + 21, VOCAB + 23], np.int64),
                         np.array([0.5, -0.5, 1.0, -4.0], np.float32)),
    }
    return vs, queries


# ---------------------------------------------------------------------------------------------------------------------
# the hybrid grid: rows, queries, bands and the fp64 ranking of tests/test_search_prior_gpu.py
def hybrid_pairs():
    """The 8 (query number, (terms, weights)) pairs; every fourth term set has signed weights."""
    return [(j, query(40 + j, m, signed=(j % 4 == 3))) for j, m in enumerate(HYBRID_MS)]


def hybrid_truth(tp, vs, d, metric):
    """x, q, S64, band, sp32 [8, N], sp64 [8, N], mag [8, N] and the fused fp64 values F [8, N] of one (metric, d)."""
    x = tp._rows(N, d, 11)
    q = tp._queries(x, len(HYBRID_MS), 12)
    S64, band = tp._truth(x, q, metric)
    pairs = hybrid_pairs()
    sp32 = np.stack([vs.f32(t, w)[0] for _, (t, w) in pairs])
    both = [vs.f64(t, w) for _, (t, w) in pairs]
    sp64, mag = np.stack([b[0] for b in both]), np.stack([b[1] for b in both])
    a = np.float64(np.float32(HYBRID_ALPHA))
    F = S64 + a * sp64 if metric == 0 else S64 - a * sp64
    return x, q, S64, band, sp32, sp64, mag, F


def hybrid_exempt(tp, F, k, metric, allowed=None):
    """(I_ref, V, nxt, the slots exempt from the id comparison): THE count of both the host and the GPU test."""
    I_ref, V, nxt = tp._topk64(F, k, metric, allowed)
    return I_ref, V, nxt, tp._exempt(I_ref, V, nxt)
