"""numpy restatement of ``include/css_synth.h`` (bit-identical to the C/HIP form).

Used by bench.py and the tests to regenerate, on the host, any row of a
synthetic index / any synthetic token sequence the device generated.
"""
from __future__ import annotations

import numpy as np

_GOLDEN = np.uint64(0x9E3779B97F4A7C15)
_M1 = np.uint64(0xBF58476D1CE4E5B9)
_M2 = np.uint64(0x94D049BB133111EB)
SYNTH_SCALE = np.float32(2.64290629e-05)


def mix64(seed: int, idx: np.ndarray) -> np.ndarray:
    idx = np.asarray(idx, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = np.uint64(seed & 0xFFFFFFFFFFFFFFFF) + _GOLDEN * (idx + np.uint64(1))
        z = (z ^ (z >> np.uint64(30))) * _M1
        z = (z ^ (z >> np.uint64(27))) * _M2
        return z ^ (z >> np.uint64(31))


def normal(seed: int, idx: np.ndarray) -> np.ndarray:
    h = mix64(seed, idx)
    m = np.uint64(0xFFFF)
    s = ((h & m).astype(np.int64) + ((h >> np.uint64(16)) & m).astype(np.int64)
         + ((h >> np.uint64(32)) & m).astype(np.int64) + (h >> np.uint64(48)).astype(np.int64) - 131070)
    return s.astype(np.float32) * SYNTH_SCALE


def uint(seed: int, idx: np.ndarray, lo: int, hi: int) -> np.ndarray:
    h = mix64(seed, idx)
    return (np.uint64(lo) + (((h >> np.uint64(32)) * np.uint64(hi - lo)) >> np.uint64(32))).astype(np.int64)


def tensor_seed(seed: int, tensor_id: int) -> int:
    return (seed ^ (tensor_id << 40) ^ 0xC55E7E11) & 0xFFFFFFFFFFFFFFFF


def rows(n: int, d: int, seed: int, first_row: int = 0) -> np.ndarray:
    """[n, d] fp32: row r, col c = normal(seed, (first_row + r) * d + c)."""
    idx = (np.arange(n, dtype=np.uint64)[:, None] + np.uint64(first_row)) * np.uint64(d) + np.arange(d, dtype=np.uint64)[None, :]
    return normal(seed, idx)


def rows_torch(n: int, d: int, seed: int, first_row: int = 0, device="cuda"):
    """``rows`` on a torch device, bit-identical (int64 arithmetic wraps like uint64; right shifts are made logical
    by masking).  Lets benchmarks and tests build derived synthetic data (clustered rows) at 10 M-row scale without
    generating 30 GB on the host."""
    import torch

    def lsr(z, sh):
        return (z >> sh) & ((1 << (64 - sh)) - 1)

    def s64(v):   # python int (uint64 value) -> the int64 with the same bits
        v &= 0xFFFFFFFFFFFFFFFF
        return v - (1 << 64) if v >= (1 << 63) else v

    idx = (torch.arange(n, dtype=torch.int64, device=device)[:, None] + first_row) * d + \
        torch.arange(d, dtype=torch.int64, device=device)[None, :]
    z = s64(seed) + s64(int(_GOLDEN)) * (idx + 1)
    z = (z ^ lsr(z, 30)) * s64(int(_M1))
    z = (z ^ lsr(z, 27)) * s64(int(_M2))
    h = z ^ lsr(z, 31)
    ssum = (h & 0xFFFF) + (lsr(h, 16) & 0xFFFF) + (lsr(h, 32) & 0xFFFF) + lsr(h, 48) - 131070
    return ssum.to(torch.float32) * float(SYNTH_SCALE)


TERM_VOCAB = 4096


def term_lists(n: int, seed: int, vocab: int = TERM_VOCAB):
    """Synthetic per-row term lists for the hybrid search, as CSR ``(offsets int64 [n + 1], tokens uint32)``: row
    lengths ``16 + integers(0, 240)``, tokens ``floor(vocab * u^3)`` with ``u`` uniform -- the cube gives a Zipf-like
    skew (term 11 of 4096 occurs in 40 % of the rows, term 2550 in 1.4 %).  Drawn as one ``[n, 255]`` matrix cut at each
    row's length, from ``numpy.random.default_rng(seed)``."""
    rng = np.random.default_rng(seed)
    dl = 16 + rng.integers(0, 240, size=n)
    tok = np.floor(vocab * rng.random((n, 255)) ** 3).astype(np.uint32)
    keep = np.arange(255)[None, :] < dl[:, None]
    off = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(dl, out=off[1:])
    return off, np.ascontiguousarray(tok[keep])


def sparse_vectors(n: int, seed: int, vocab: int = TERM_VOCAB, lattice: bool = False):
    """Synthetic per-row sparse vectors, as CSR ``(offsets int64 [n + 1], terms uint32, weights float32)``: the row
    sizes and the ``u^3`` term skew of ``term_lists`` (same draws from ``numpy.random.default_rng(seed)``), the terms
    de-duplicated per row and ascending, then one weight per kept entry, ``log1p`` of a standard exponential draw (a
    draw that rounds to 0 becomes the smallest positive normal float32).  ``lattice=True``: the weights are multiples of 1/8
    in ``(0, 4]`` instead, so that sums of products with lattice query weights are exact in fp32."""
    rng = np.random.default_rng(seed)
    dl = 16 + rng.integers(0, 240, size=n)
    tok = np.floor(vocab * rng.random((n, 255)) ** 3).astype(np.int64)
    keep = np.arange(255)[None, :] < dl[:, None]
    key = np.unique((np.arange(n, dtype=np.int64)[:, None] << 32 | tok)[keep])
    off = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(key >> 32, minlength=n), out=off[1:])
    if lattice:
        w = (rng.integers(1, 33, size=key.shape[0]) / 8.0).astype(np.float32)
    else:
        w = np.maximum(np.log1p(rng.standard_exponential(key.shape[0])).astype(np.float32), np.finfo(np.float32).tiny)
    return off, (key & 0xFFFFFFFF).astype(np.uint32), w


TOKEN_EDGE_LENGTHS = (0, 1, 15, 16, 17, 63, 64, 65, 512)


def token_matrices(n: int, P: int, seed: int, lattice=False, max_len: int = 40):
    """Synthetic per-row token matrices, as CSR ``(offsets int64 [n + 1] in tokens, tokens uint16 [E, P] of bf16 bits,
    P)``: row lengths ``integers(0, max_len + 1)`` from ``numpy.random.default_rng(seed)`` with the first rows forced
    to ``TOKEN_EDGE_LENGTHS`` (empty, one token, around the 16-token tile and its multiples, the longest row the index
    takes), then Gaussian rows scaled to unit length and rounded to bf16.  ``lattice``: the components are ``{-8 .. 8}
    / 8`` instead (``True`` or ``"E"``) or ``{-1, 0, 1}`` (``"T"``), exact in bf16, so that every dot product and every
    MaxSim sum is exact in fp32."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, max_len + 1, size=n)
    edge = np.asarray(TOKEN_EDGE_LENGTHS[:n], dtype=lens.dtype)
    lens[:edge.shape[0]] = edge
    off = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(lens, out=off[1:])
    E = int(off[-1])
    if lattice == "T":
        x = rng.integers(-1, 2, size=(E, P)).astype(np.float32)
    elif lattice:
        x = (rng.integers(-8, 9, size=(E, P)) / 8.0).astype(np.float32)
    else:
        x = rng.standard_normal((E, P))
        x = (x / np.maximum(np.linalg.norm(x, axis=1, keepdims=True), 1e-30)).astype(np.float32)
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return off, ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16), int(P)


def clustered_token_matrices(n: int, P: int, seed: int, ncentres: int = 256, spread: float = 0.25, max_len: int = 40):
    """Token matrices with the structure a token codec can find, in the CSR form and with the row lengths of
    ``token_matrices``: ``ncentres`` Gaussian unit centres, every token one of them (uniformly drawn) plus Gaussian noise
    of total length ``spread`` in expectation, scaled to unit length and rounded to bf16.  Gaussian unit vectors in 128
    dimensions have no such structure: every token is nearly orthogonal to every centroid."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, max_len + 1, size=n)
    edge = np.asarray(TOKEN_EDGE_LENGTHS[:n], dtype=lens.dtype)
    lens[:edge.shape[0]] = edge
    off = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(lens, out=off[1:])
    E = int(off[-1])
    centres = rng.standard_normal((ncentres, P))
    centres /= np.linalg.norm(centres, axis=1, keepdims=True)
    x = centres[rng.integers(0, ncentres, size=E)] + rng.standard_normal((E, P)) * (spread / np.sqrt(P))
    x = (x / np.maximum(np.linalg.norm(x, axis=1, keepdims=True), 1e-30)).astype(np.float32)
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return off, ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16), int(P)


def query_terms(j: int, count: int = 4, vocab: int = TERM_VOCAB) -> np.ndarray:
    """The distinct values, in order of first occurrence, of ``floor(vocab * default_rng(500 + j).random(count)^3)``."""
    t = np.floor(vocab * np.random.default_rng(500 + j).random(count) ** 3).astype(np.int64)
    return t[np.sort(np.unique(t, return_index=True)[1])]
