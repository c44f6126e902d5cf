"""The inputs of tests/test_tokens_index_gpu.py, stated once, so that tests/test_tokens_index_host.py can prove with numpy
alone that they make the exact checks of the GPU tests bind.  Nothing here touches a device."""
import functools

import numpy as np

import late_cases as lt
import lattice_cases as lc
from claude_semantic_search_amd import synth
from claude_semantic_search_amd.late_interaction import bf16_to_f32, f32_to_bf16
from tokens_fakes import Matrices

N = 3001                     # not a multiple of 16, 64 or 256: the last turn, run and slice are partial
D = 64                       # the dense rows the matrices ride on
T_PART = 2600                # rows [T_PART, N) have no matrix in the "rows >= T" cases
WIDTHS = (32, 64, 96, 128)
KS = (1, 10, 128)
FAMILIES = ("T", "E")
QUERY_LENS = lt.QUERY_LENS   # 1, 15, 16, 17, 32, 64
ID_BASE = 10 ** 9
PLANT_QUERY = 3              # the query (17 tokens) whose best possible doc is planted twice: a tie at rank 1
PLANTS = (1000, 2000)
EDGE = synth.TOKEN_EDGE_LENGTHS


def to_bits(x):
    """uint16 bf16 bits of float32 values that are exact in bf16."""
    return lt.to_bf16(x)


@functools.lru_cache(maxsize=16)
def lattice(family, P):
    """(Matrices over N rows, [query uint16 [mq, P] per QUERY_LENS]) of one (family, P).  The docs at PLANTS are
    sign(q) of query PLANT_QUERY, token for token: with components of size at most 1 no doc can score higher, so the
    two tie at rank 1."""
    seed = {"T": 5000, "E": 6000}[family] + P
    off, tok, _ = synth.token_matrices(N, P, seed, lattice=family)
    qs = [to_bits(lc.FAMILIES[family](m, P, seed + 100 + i)) for i, m in enumerate(QUERY_LENS)]
    mats = Matrices(off, tok).mats()
    plant = to_bits(np.sign(bf16_to_f32(qs[PLANT_QUERY])).astype(np.float32))
    for r in PLANTS:
        mats[r] = plant
    return Matrices.of(mats, P), qs


@functools.lru_cache(maxsize=8)
def gaussian(P):
    """(Matrices over N rows, queries) of Gaussian unit rows rounded to bf16."""
    off, tok, _ = synth.token_matrices(N, P, 7000 + P)
    rng = np.random.default_rng(7100 + P)
    qs = []
    for m in QUERY_LENS:
        x = rng.standard_normal((m, P))
        qs.append(f32_to_bf16((x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)))
    return Matrices(off, tok), qs


def half_mask():
    return np.random.default_rng(8).random(N) < 0.5


def negative_case(P):
    """(Matrices, query): docs with components in {0 .. 8} / 8 with a 1 in component 0, a query of two tokens with
    components in {-8 .. -1} / 8: every dot is negative, every score is negative, and the ranking still holds."""
    rng = np.random.default_rng(9000 + P)
    off, _, _ = synth.token_matrices(N, P, 9000 + P, lattice=True)
    tok = (rng.integers(0, 9, size=(int(off[-1]), P)) / 8.0).astype(np.float32)
    tok[:, 0] = 1.0
    q = (-rng.integers(1, 9, size=(2, P)) / 8.0).astype(np.float32)
    return Matrices(off, to_bits(tok)), to_bits(q)


def bound(q, ms):
    """float64 [n]: 2^-23 mq (P + mq) c per row, c the largest ||q_s|| ||d_t|| of the pair -- the derived bound of
    tests/test_maxsim_gpu.py; 0 for a row without tokens."""
    mq, P = q.shape
    qn = np.linalg.norm(bf16_to_f32(q).astype(np.float64), axis=1).max()
    dn = np.linalg.norm(bf16_to_f32(ms.tok).astype(np.float64), axis=1)
    out = np.zeros(ms.n)
    live = np.flatnonzero(ms.lens > 0)
    out[live] = np.maximum.reduceat(dn, ms.off[:-1][live])
    return 2.0 ** -23 * mq * (P + mq) * qn * out
