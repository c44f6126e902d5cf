"""TEST SUPPORT, NOT PRODUCT CODE -- token matrices for the MaxSim tests (css_encoder_maxsim).

Lattice matrices (families T and E of ``lattice_cases.py``) make every product and every partial sum of a dot product
exact in fp32, and so the sum of the per-token maxima: the float64 truth of ``maxsim_numpy`` IS the fp32 result, bit for
bit.  Gaussian matrices are unit rows rounded to bf16, with a derived bound.  Plain module; nothing here touches the GPU.
"""
import numpy as np

import lattice_cases as lc
from claude_semantic_search_amd.late_interaction import bf16_to_f32, f32_to_bf16, maxsim_numpy

WIDTHS = (32, 64, 96, 128, 384, 768)
QUERY_LENS = (1, 15, 16, 17, 32, 64)
DOC_LENS = (1, 15, 16, 17, 63, 64, 65, 512)


def to_bf16(x):
    """uint16 bit patterns; the test's inputs must be exact in bf16."""
    b = f32_to_bf16(x)
    assert np.array_equal(bf16_to_f32(b), np.asarray(x, dtype=np.float32))
    return b


def lattice_mats(family, P, seed):
    """``(q_mats, d_mats)`` as float32: one query per QUERY_LENS, one doc per DOC_LENS."""
    q = [lc.FAMILIES[family](m, P, seed + 10 * i) for i, m in enumerate(QUERY_LENS)]
    d = [lc.FAMILIES[family](m, P, seed + 1000 + 10 * j) for j, m in enumerate(DOC_LENS)]
    return q, d


def keep_variants(d_mats):
    """Per doc one keep vector: the first token dropped (65 tokens), the last (64), one whole 16-token tile (512), all
    but one (63), the last token of a partial tile alone (17); the other docs keep everything."""
    keep = [np.ones(m.shape[0], dtype=np.uint8) for m in d_mats]
    for k in keep:
        n = k.size
        if n == 65:
            k[0] = 0
        elif n == 64:
            k[-1] = 0
        elif n == 512:
            k[32:48] = 0
        elif n == 63:
            k[:] = 0
            k[40] = 1
        elif n == 17:
            k[:] = 0
            k[16] = 1
    return keep


def truth(q_mats, d_mats, pairs, keep=None):
    """float64 MaxSim of every pair, and its float32 image."""
    t = np.array([maxsim_numpy(q_mats[i], d_mats[j], None if keep is None else keep[j]) for i, j in pairs],
                 dtype=np.float64)
    return t, t.astype(np.float32)


def scrambled_pairs(nq, nd, skip_q, skip_d):
    """Every (query, doc) without query ``skip_q`` and doc ``skip_d``, in reverse order, then the first five again."""
    pr = [(i, j) for i in range(nq) for j in range(nd) if i != skip_q and j != skip_d][::-1]
    return pr + pr[:5]


def gaussian_mats(P, seed):
    """Unit Gaussian rows rounded to bf16 (float32 values of the bf16 rows), shapes as ``lattice_mats``."""
    rng = np.random.default_rng(seed)

    def unit(m):
        x = rng.standard_normal((m, P))
        x /= np.linalg.norm(x, axis=1, keepdims=True)
        return bf16_to_f32(f32_to_bf16(x.astype(np.float32)))

    return [unit(m) for m in QUERY_LENS], [unit(m) for m in DOC_LENS]
