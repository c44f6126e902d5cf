"""GPU: the asymmetric search of the binary store (css_bin_search_asym*, k_bin_asym_prep / k_bin_asym_topk in
csrc/css_binary.h) against the numpy restatement of binary.py.  Everything is integers: every comparison is array_equal."""
import functools

import numpy as np
import pytest

from claude_semantic_search_amd.binary import (IndexBinaryFlat, asym_scores_numpy, quantize_queries_numpy,
                                               search_asym_numpy)

pytestmark = pytest.mark.gpu

DIMS = (32, 96, 768, 8192)   # one word, an odd number of words, the usual (queries in registers), the maximum (in LDS)
N = 5000                     # 79 steps of 64 rows, the last one partial
KS = (1, 10, 128)


@functools.lru_cache(maxsize=None)
def store(d):
    """(store of N uniform random codes with row 0 all ones and row 1 all zeros, its codes): built once per d."""
    rows = np.random.default_rng(100 + d).integers(0, 256, size=(N, d // 8), dtype=np.uint8)
    rows[0], rows[1] = 255, 0
    ix = IndexBinaryFlat(d)
    ix.add(rows)
    return ix, rows


@functools.lru_cache(maxsize=None)
def queries(d, family):
    """(33 int8 queries, their scores).  "signs": components in {-1, 0, 1}, few distinct scores, so ties straddle rank k.
    "full": the whole of int8, query 0 all -128 and query 1 all 127: at d = 8192 the scores reach +-2^20."""
    rng = np.random.default_rng(200 + d)
    if family == "signs":
        q8 = rng.integers(-1, 2, size=(33, d), dtype=np.int8)
    else:
        q8 = rng.integers(-128, 128, size=(33, d), dtype=np.int8)
        q8[0], q8[1] = -128, 127
    s = asym_scores_numpy(q8, store(d)[1])
    if family == "signs" and d == 32:
        t = -np.sort(-s, axis=1)
        assert all((t[:, k - 1] == t[:, k]).sum() > (16 if k >= 10 else 0) for k in KS)
    if family == "full" and d == 8192:
        assert s[0, 0] == -2 ** 20 and s[0, 1] == 2 ** 20
    s.setflags(write=False)
    return q8, s


@functools.lru_cache(maxsize=None)
def allow_mask():
    m = np.random.default_rng(7).random(N) < 0.4
    m[4990:] = True   # (rows of the partial last step among them)
    return m


@functools.lru_cache(maxsize=None)
def reference(d, family, k, masked):
    return search_asym_numpy(queries(d, family)[1], k, allow_mask() if masked else None)


@pytest.mark.parametrize("masked", (False, True))
@pytest.mark.parametrize("waves", (0, 1, 3))   # a wave walks 1, 79 or 27 steps: the merge, the threshold and the insert path
@pytest.mark.parametrize("family", ("signs", "full"))
@pytest.mark.parametrize("d", DIMS)
def test_search_is_the_restatement(d, family, waves, masked):
    ix, q8 = store(d)[0], queries(d, family)[0]
    ix.set_waves(waves)
    try:
        for k in KS:
            Dr, Ir = reference(d, family, k, masked)
            for nq in (1, 3, 16, 17, 33):
                D, I = ix.search_asym(q8[:nq], k, allow_mask() if masked else None)
                assert D.dtype == np.int32 and I.dtype == np.int64 and ix.last_passes == -(-nq // 16)
                assert np.array_equal(I, Ir[:nq]) and np.array_equal(D, Dr[:nq]), (k, nq)
    finally:
        ix.set_waves(0)


@pytest.mark.parametrize("d", DIMS)
def test_forms_agree(d):
    """The float form is search_asym of quantize_queries_numpy's int8 (a zero query and one with a denormal maximum
    among Gaussian ones); the _dev forms give the bytes of the host forms."""
    import torch

    ix, rows = store(d)
    q = np.random.default_rng(300 + d).standard_normal((19, d)).astype(np.float32)
    q[3] = 0
    q[5] = 0
    q[5, ::7] = 1e-39
    q8 = quantize_queries_numpy(q)[0]
    assert not q8[3].any() and not q8[5].any() and (np.abs(q8).max(axis=1)[[0, 18]] == 127).all()
    for mask in (None, allow_mask()):
        Dr, Ir = search_asym_numpy(asym_scores_numpy(q8, rows), 10, mask)
        for got in (ix.search_asym(q8, 10, mask), ix.search_asym_float(q, 10, mask), ix.search_asym_dev(torch.from_numpy(q).cuda(), 10, mask),
                    ix.search_asym_i8_dev(torch.from_numpy(q8).cuda(), 10, mask)):
            Dg, Ig = (np.asarray(t.cpu() if hasattr(t, "cpu") else t) for t in got)
            assert Dg.dtype == np.int32 and np.array_equal(Dg, Dr) and np.array_equal(Ig, Ir)


@pytest.mark.parametrize("waves", (0, 2))
@pytest.mark.parametrize("n", (1, 255, 257))
def test_padding(n, waves):
    """An empty store answers with padding; k = 128 with n = 1 rows, or with the 1 + n // 3 rows a mask leaves, pads."""
    rng = np.random.default_rng(n)
    rows, q8 = rng.integers(0, 256, size=(n, 12), dtype=np.uint8), rng.integers(-128, 128, size=(3, 96), dtype=np.int8)
    with IndexBinaryFlat(96) as ix:
        D, I = ix.search_asym(q8, 5)
        assert (D == -2 ** 31).all() and (I == -1).all() and ix.last_passes == 0
        ix.add(rows)
        ix.set_waves(waves)
        for mask in (None, np.arange(n) % 3 == 0):
            D, I = ix.search_asym(q8, 128, mask)
            Dr, Ir = search_asym_numpy(asym_scores_numpy(q8, rows), 128, mask)
            assert np.array_equal(I, Ir) and np.array_equal(D, Dr)
            assert (I[:, -1] == -1).all() or (mask is None and n > 128)
