"""The inputs of tests/test_tokens_codec_gpu.py, stated once, so that tests/test_tokens_codec_host.py can prove with numpy
alone that they make the exact checks of the GPU tests bind.  Nothing here touches a device.

Lattice cases: tokens and centroids have components in {-8 .. 8} / 8 (duplicate centroids among them), weights are
multiples of 1/8 in [-1, 1], cutoffs lie ON lattice values.  Every dot, residual and decoded value is then exact:
centroid + weight is a multiple of 1/8 within +-2, a bf16 value, and a score is a sum of at most 64 * 128 products that
are multiples of 1/64 of size at most 2 -- below 2^24 units of 1/64, exact in fp32 in any order."""
import functools

import numpy as np

from claude_semantic_search_amd import synth
from claude_semantic_search_amd.flat_index import TokenCodec, bf16_to_f32, f32_to_bf16_rne
from tokens_fakes import Matrices

N = 500                      # docs; not a multiple of 16 or 64: the last turn and run are partial
D = 64                       # the dense rows the matrices ride on
T_PART = 430                 # rows [T_PART, N) have no matrix in the "rows >= T" cases
WIDTHS = (32, 64, 96, 128)
BITS = (1, 2, 4)
CENTROIDS = (1, 17, 256, 300)
QUERY_LENS = (1, 16, 17, 32, 64)
KS = (1, 10, 128)
EDGE = (0, 1, 15, 16, 17, 33, 512)
POOL = 60                    # distinct matrices behind the N docs: equal docs tie in score
ID_BASE = 10 ** 9

CUTOFFS = {1: np.array([0.0], np.float32),
           2: np.array([-0.125, 0.0, 0.125], np.float32),
           4: (np.arange(-7, 8) / 8.0).astype(np.float32)}
WEIGHTS = {1: np.array([-0.125, 0.125], np.float32),
           2: np.array([-0.25, -0.125, 0.125, 0.25], np.float32),
           4: (np.arange(-8, 8) / 8.0).astype(np.float32)}


def to_bits(x):
    """uint16 bf16 bits of float32 values that are exact in bf16."""
    x = np.ascontiguousarray(x, np.float32)
    assert not (x.view(np.uint32) & 0xFFFF).any()
    return (x.view(np.uint32) >> 16).astype(np.uint16)


def lattice_codec(P, nbits, C, seed=0):
    rng = np.random.default_rng(100 * P + 10 * nbits + C + seed)
    cent = (rng.integers(-8, 9, size=(C, P)) / 8.0).astype(np.float32)
    for a, b in ((0, C // 2), (3, C - 1), (5, 6)):   # duplicates: the lower id must win
        if a < b < C:
            cent[b] = cent[a]
    return TokenCodec(cent, nbits, CUTOFFS[nbits].copy(), WEIGHTS[nbits].copy())


def _lengths(n, seed):
    lens = np.random.default_rng(seed).integers(0, 41, size=n)
    lens[:len(EDGE)] = EDGE
    return lens


@functools.lru_cache(maxsize=64)
def lattice(P, nbits, C):
    """(codec, Matrices over N rows, [query uint16 [mq, P] per QUERY_LENS]).  A token is a centroid plus lattice noise in
    {-2 .. 2} / 8, clipped to [-1, 1]; every eighth token is a copy of one of the duplicated centroids, so its best
    centroid is tied.  The docs are drawn from POOL distinct matrices, so scores tie across ranks."""
    codec = lattice_codec(P, nbits, C)
    rng = np.random.default_rng(7 * P + nbits + 1000 * C)
    lens = _lengths(POOL, 11 + P)
    pool = []
    for m in lens:
        base = codec.centroids[rng.integers(0, C, size=m)]
        t = np.clip(base + rng.integers(-2, 3, size=(m, P)) / 8.0, -1.0, 1.0).astype(np.float32)
        dup = np.flatnonzero(np.arange(m) % 8 == 7)
        t[dup] = codec.centroids[0]
        pool.append(to_bits(t))
    pick = np.concatenate([np.arange(len(EDGE)), rng.integers(len(EDGE), POOL, size=N - len(EDGE))])
    pick[-1] = EDGE.index(512)   # the longest doc wins most queries: its twin ties with it at rank 1
    ms = Matrices.of([pool[i] for i in pick], P)
    qs = [to_bits((rng.integers(-8, 9, size=(m, P)) / 8.0).astype(np.float32)) for m in QUERY_LENS]
    return codec, ms, qs


def negative_case(P, nbits):
    """(codec, Matrices, query): centroids and tokens in {0 .. 8} / 8 with a 1 in component 0, weights >= 0, a query of
    two tokens with components in {-8 .. -1} / 8: every decoded component is >= 0 with component 0 >= 1, so every dot and
    every score is negative."""
    rng = np.random.default_rng(9000 + P + nbits)
    cent = (rng.integers(0, 9, size=(17, P)) / 8.0).astype(np.float32)
    cent[:, 0] = 1.0
    codec = TokenCodec(cent, nbits, CUTOFFS[nbits].copy(), np.abs(WEIGHTS[nbits]))
    lens = _lengths(N, 5)
    off = np.concatenate([[0], np.cumsum(lens)])
    tok = (rng.integers(0, 9, size=(int(off[-1]), P)) / 8.0).astype(np.float32)
    tok[:, 0] = 1.0
    q = (-rng.integers(1, 9, size=(2, P)) / 8.0).astype(np.float32)
    return codec, Matrices(off, to_bits(tok)), to_bits(q)


def half_mask():
    return np.random.default_rng(8).random(N) < 0.5


def unit_queries(P, seed):
    rng = np.random.default_rng(seed)
    qs = []
    for m in QUERY_LENS:
        x = rng.standard_normal((m, P))
        qs.append(f32_to_bf16_rne((x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)))
    return qs


@functools.lru_cache(maxsize=8)
def arbitrary(kind, P):
    """(Matrices over N rows, queries) of unit tokens rounded to bf16: "clustered" around a few hundred centres
    (synth.clustered_token_matrices) or "gaussian" (synth.token_matrices)."""
    if kind == "clustered":
        off, tok, _ = synth.clustered_token_matrices(N, P, 300 + P, ncentres=200)
    else:
        off, tok, _ = synth.token_matrices(N, P, 400 + P)
    return Matrices(off, tok), unit_queries(P, 500 + P)


def dots64(codec, tok):
    """float64 [E, C] dots of bf16 tokens with the codec's centroids."""
    return bf16_to_f32(tok).astype(np.float64) @ codec.centroids.astype(np.float64).T


def encode64(codec, tok):
    """The float64 restatement of encode: (codes, buckets uint8 [E, P]) -- exact on lattice inputs."""
    d = dots64(codec, tok)
    codes = d.argmax(axis=1).astype(np.uint16)            # (the first maximum: ties to the lower id)
    r = bf16_to_f32(tok).astype(np.float64) - codec.centroids[codes].astype(np.float64)
    buckets = (codec.cutoffs.astype(np.float64)[None, None, :] < r[:, :, None]).sum(axis=2).astype(np.uint8)
    return codes, buckets


def decode64(codec, codes, buckets):
    """float64 decode, exact on lattice inputs: centroid + weight."""
    return codec.centroids[codes].astype(np.float64) + codec.weights.astype(np.float64)[buckets]


def assign_bound(P, tok, codec):
    """How far the chosen centroid's exact dot may fall short of the exact maximum: float64 [E].  An fp32 dot of P exact
    products (both operands are bf16) in any order errs by at most 2^-23 P c, with c = ||d|| ||c|| bounding every sum
    of |products| -- the per-dot bound of tests/test_maxsim_gpu.py.  The device picks the largest fp32 dot, so the
    shortfall is at most one such error on each of the two dots compared: 2 * 2^-23 P ||d|| max ||c||."""
    dn = np.linalg.norm(bf16_to_f32(tok).astype(np.float64), axis=1)
    cn = np.linalg.norm(codec.centroids.astype(np.float64), axis=1).max()
    return 2.0 * 2.0 ** -23 * P * dn * cn
