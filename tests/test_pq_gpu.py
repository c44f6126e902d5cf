"""GPU: the product-quantized row store (css_pq_*, csrc/css_pq.h) against the numpy restatement of pq.ProductQuantizer:
codes and scores bit for bit on lattice inputs, within derived bounds on Gaussian ones, the same bytes whatever the
batch, the order of the adds and the form, and through ``IndexFlat.search_fde_pq``."""
import ctypes
import functools

import numpy as np
import pytest

import late_cases as late
import lattice_cases as lc
from claude_semantic_search_amd import _native as nat
from claude_semantic_search_amd.flat_index import IndexFlatIP, bf16_to_f32, f32_to_bf16_rne, search_rerank_maxsim_numpy
from claude_semantic_search_amd.muvera import FixedDimensionalEncoding
from claude_semantic_search_amd.pq import IndexPQ, ProductQuantizer, search_numpy, train_product_quantizer

pytestmark = pytest.mark.gpu

DIMS = (32, 96, 768, 8192)   # one K step, a partial slice of 16 sub-quantizers, several slices, the maximum
N = 2999
U = 2.0 ** -24


def lattice_pq(d):
    """Centroids in {-8 .. 8} / 8 with every centroid c >= 128 a copy of centroid c - 128 (so that ties occur in every
    sub-quantizer) and, in sub-quantizer 0, 16 more copies of centroid 1."""
    cb = lc.family_E(d // 8 * 256, 8, 50 + d).reshape(d // 8, 256, 8)
    cb[0, 40:56] = cb[0, 1]
    cb[:, 128:] = cb[:, :128]
    return ProductQuantizer(d, cb)


def gaussian_pq(d, seed):
    rng = np.random.default_rng(seed)
    return ProductQuantizer(d, rng.standard_normal((d // 8, 256, 8)).astype(np.float32)), rng


@functools.lru_cache(maxsize=None)
def lattice_encoded(d):
    """(quantizer, 1000 lattice rows, their codes by the float32 restatement): computed once per d."""
    pq, x = lattice_pq(d), lc.lattice_rows("E", 1000, d, 60 + d)
    want = pq.encode_numpy(x)
    want.setflags(write=False)
    return pq, x, want


@functools.lru_cache(maxsize=None)
def lattice_store(d):
    """(store of N lattice rows, 33 queries, their float64 scores): built once per d; the codes are the device's."""
    pq, x = lattice_pq(d), lc.lattice_rows("E", N, d, 70 + d)
    ix = IndexPQ(d, pq)
    ix.add(x)
    q = lc.lattice_queries("E", 33, d, 80 + d)
    s = pq.scores_numpy(q, ix.get_codes())
    s.setflags(write=False)
    return ix, q, s


@pytest.mark.parametrize("n", (1, 15, 17, 1000))
@pytest.mark.parametrize("d", DIMS)
def test_encode_lattice_exact(d, n):
    """Every difference, square and partial sum is a multiple of 1/64 below 2^11: exact in fp32.  Each centroid has a
    copy 128 places on, so every argmin is a tie and must be the lower one."""
    pq, x, want = lattice_encoded(d)
    assert (want < 128).all()
    with IndexPQ(d, pq) as ix:
        ix.add(x[:n])
        assert ix.ntotal == n and np.array_equal(ix.get_codes(), want[:n])


def test_encode_gaussian():
    """d = 96, 1000 unit Gaussian rows, Gaussian codebooks.  The device's codes are the float32 restatement's.  Against
    float64: a computed distance is sum_j fl(fl(t_j)^2) with t_j = fl(x_j - c_j), summed by 7 additions (0 + p is
    exact), so every non-negative term carries at most (1 + u)^10, u = 2^-24, and |s^ - s| <= g s with g = 10 u / (1 -
    10 u).  The device can prefer c' to float64's c only if s^(c') <= s^(c), which needs s(c') - s(c) <= g (s(c') +
    s(c)): that is asserted of every differing code, and their share is capped at 1 %.  (On the CPU, with the two
    restatements alone, this seed gives 0 differing codes of 12 000.)"""
    pq, rng = gaussian_pq(96, 21)
    x = rng.standard_normal((1000, 96)).astype(np.float32)
    with IndexPQ(96, pq) as ix:
        ix.add(x)
        got = ix.get_codes()
    assert np.array_equal(got, pq.encode_numpy(x))
    ref = pq.encode_numpy(x, np.float64)
    rows, ms = np.nonzero(got != ref)
    print(f"codes differing from float64: {rows.size} of {got.size}")
    assert rows.size <= 0.01 * got.size
    g = 10 * U / (1 - 10 * U)
    sub = x.reshape(-1, 12, 8).astype(np.float64)[rows, ms]
    cb = pq.codebooks.astype(np.float64)
    s_got = ((sub - cb[ms, got[rows, ms]]) ** 2).sum(axis=1)
    s_ref = ((sub - cb[ms, ref[rows, ms]]) ** 2).sum(axis=1)
    assert (s_got - s_ref <= g * (s_got + s_ref)).all()


@pytest.mark.parametrize("masked", (False, True))
@pytest.mark.parametrize("k", (1, 10, 128))
@pytest.mark.parametrize("nq", (1, 3, 16, 17, 33))
@pytest.mark.parametrize("d", DIMS)
def test_search_lattice_exact(d, nq, k, masked):
    """Products and partial sums are multiples of 1/64 below 2^13: the fp32 scores are float64's, and (D, I) is the
    lexsort with no tolerance.  The rows hold a block of 40 copies, so equal scores meet in the lists."""
    ix, q, s = lattice_store(d)
    allow = np.random.default_rng(d + nq).random(N) < 0.4 if masked else None
    D, I = ix.search(q[:nq], k, allow=allow)
    Dw, Iw = search_numpy(s[:nq], k, allow)
    assert ix.last_passes == (nq + 15) // 16
    assert np.array_equal(I, Iw) and np.array_equal(D, Dw)
    assert np.unique(s[0]).size < N - 30


@pytest.mark.parametrize("d", (96, 768, 8192))
def test_scores_gaussian(d):
    """Gaussian queries and codebooks, 2999 random codes, k = 20.  The products of bf16 operands are exact in fp32, and
    d - 1 fp32 additions in ANY order stay within g_d sum_i |q^_i x^_i| of the float64 sum, g_d = d u / (1 - d u): that
    holds of every returned D.  With B the largest such bound over the rows of a query, the j-th largest computed and
    the j-th largest true score differ by at most B (order statistics under a perturbation of at most B), and the
    computed score of the returned row is within B of its true score: a returned id may differ from the float64
    ranking's only where the two true scores are within 2 B."""
    pq, rng = gaussian_pq(d, 31 + d)
    codes = rng.integers(0, 256, size=(N, d // 8), dtype=np.uint8)
    q = rng.standard_normal((17, d)).astype(np.float32)
    with IndexPQ(d, pq) as ix:
        ix.add_codes(codes)
        D, I = ix.search(q, 20)
    s = pq.scores_numpy(q, codes)
    qa =np.abs(bf16_to_f32(f32_to_bf16_rne(q)).reshape(q.shape).astype(np.float64))
    bound = d * U / (1 - d * U) * (qa @ np.abs(pq.decode_numpy(codes).astype(np.float64)).T)
    rows = np.arange(17)[:, None]
    err = np.abs(D.astype(np.float64) - s[rows, I])
    print(f"d={d}: max |D - float64| = {err.max():.3e}, smallest bound = {bound[rows, I].min():.3e}")
    assert (err <= bound[rows, I]).all()
    _, I64 = search_numpy(s, 20)
    assert (np.abs(s[rows, I] - s[rows, I64]) <= 2 * bound.max(axis=1, keepdims=True)).all()


def test_independence():
    """One query alone is the same query inside a batch of 33; two adds are one add; add_codes(get_codes()) gives the
    same search; the _dev forms give the bytes of the host forms."""
    import torch

    d, k = 768, 10
    pq, rng = gaussian_pq(d, 41)
    x = rng.standard_normal((1500, d)).astype(np.float32)
    q = rng.standard_normal((33, d)).astype(np.float32)
    with IndexPQ(d, pq) as one, IndexPQ(d, pq) as two, IndexPQ(d, pq) as third, IndexPQ(d, pq) as dev:
        one.add(x)
        two.add(x[:700])
        two.add(x[700:])
        codes = one.get_codes()
        third.add_codes(codes)
        dev.add_dev(torch.from_numpy(x[:100]).cuda())   # (the second add grows the store behind the first)
        dev.add_dev(torch.from_numpy(x[100:]).cuda())
        assert np.array_equal(two.get_codes(), codes) and np.array_equal(dev.get_codes(), codes)
        D, I = one.search(q, k)
        for b in (0, 15, 16, 32):
            D1, I1 = one.search(q[b:b + 1], k)
            assert D1.tobytes() == D[b:b + 1].tobytes() and I1.tobytes() == I[b:b + 1].tobytes()
        for other in (two, third):
            D2, I2 = other.search(q, k)
            assert D2.tobytes() == D.tobytes() and I2.tobytes() == I.tobytes()
        allow = rng.random(1500) < 0.5
        Dm, Im = one.search(q, k, allow=allow)
        Dd, Id = dev.search_dev(torch.from_numpy(q).cuda(), k, allow=allow)
        torch.cuda.synchronize()
        assert Dd.cpu().numpy().tobytes() == Dm.tobytes() and Id.cpu().numpy().tobytes() == Im.tobytes()


@pytest.mark.parametrize("d", (32, 96, 768))
def test_reconstruct(d):
    pq, rng = gaussian_pq(d, 51)
    codes = rng.integers(0, 256, size=(333, d // 8), dtype=np.uint8)
    with IndexPQ(d, pq) as ix:
        ix.add_codes(codes[:100])
        ix.add_codes(codes[100:])
        assert np.array_equal(ix.reconstruct_n(), pq.decode_numpy(codes))
        assert np.array_equal(ix.reconstruct_n(65, 130), pq.decode_numpy(codes[65:195]))
        assert np.array_equal(ix.get_codes(99, 3), codes[99:102])


def test_train_product_quantizer():
    """Codebooks from the index's k-means: bf16-exact, a function of the seed, and usable as they are."""
    x = np.random.default_rng(71).standard_normal((600, 32)).astype(np.float32)
    a, b = train_product_quantizer(x, niter=2, seed=3), train_product_quantizer(x, niter=2, seed=3)
    assert a.codebooks.shape == (4, 256, 8) and a.codebooks.tobytes() == b.codebooks.tobytes()
    assert np.array_equal(bf16_to_f32(f32_to_bf16_rne(a.codebooks)).reshape(4, 256, 8), a.codebooks)
    with IndexPQ(32, a) as ix:
        ix.add(x)
        assert np.array_equal(ix.get_codes(), a.encode_numpy(x))


def test_search_fde_pq():
    """The composed calls on a small store: the pool from the codes of the encodings, the MaxSim of its rows, the
    ranking of search_rerank_maxsim_numpy."""
    P, k, fetch = 64, 3, 8
    queries, docs = late.gaussian_mats(P, 61)
    with FixedDimensionalEncoding(P, 3, 16, 4) as fde:
        flat = IndexFlatIP(fde.dim)
        flat.add_fde(fde, docs)
        pq = ProductQuantizer(fde.dim, np.random.default_rng(62).standard_normal((fde.dim // 8, 256, 8)).astype(np.float32) / 4)
        with IndexPQ(fde.dim, pq) as ix:
            ix.add(fde.encode_documents(docs))
            got = flat.search_fde_pq(fde, ix, queries, k, fetch)
            S0, I0 = ix.search(fde.encode_queries(queries), fetch)
            want = search_rerank_maxsim_numpy(S0, I0, flat.maxsim_ids_batch(queries, I0), k)
        flat.close()
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, want))
    assert (got[1][:, 0] >= 0).all()


def test_c_refusals():
    """Each refusal names the offending argument and leaves the store as it was."""
    lib, pq = nat.lib(), lattice_pq(32)
    x = np.zeros((4, 32), dtype=np.float32)
    D, I = np.zeros((2, 200), dtype=np.float32), np.zeros((2, 200), dtype=np.int64)
    with IndexPQ(32, pq) as ix:
        h = ix._handle()
        ix.add(x)

        def refused(rc, word):
            assert rc == nat.CSS_ERR_INVALID and word in nat.last_error(), nat.last_error()
            assert ix.ntotal == 4

        refused(lib.css_pq_add(h, x.ctypes.data, -1), "n < 0")
        refused(lib.css_pq_add(h, None, 1), "x is NULL")
        x[2, 9] = np.inf
        refused(lib.css_pq_add(h, x.ctypes.data, 4), "component 9 of row 2 is infinite")
        x[2, 9] = np.nan
        refused(lib.css_pq_search(h, x.ctypes.data, 4, 1, None, D.ctypes.data, I.ctypes.data), "component 9 of query 2 is NaN")
        x[2, 9] = 0.0
        refused(lib.css_pq_search(h, x.ctypes.data, 2, 129, None, D.ctypes.data, I.ctypes.data), "k=129 outside [1, 128]")
        refused(lib.css_pq_search(h, x.ctypes.data, 0, 1, None, D.ctypes.data, I.ctypes.data), "nq=0 outside")
        refused(lib.css_pq_search(h, x.ctypes.data, 2, 1, None, None, I.ctypes.data), "NULL buffer")
        refused(lib.css_pq_get_codes(h, 2, 3, D.ctypes.data), "rows [2, 5) outside [0, 4)")
        refused(lib.css_pq_reconstruct(h, -1, 1, D.ctypes.data), "rows [-1, 0) outside [0, 4)")
    out = ctypes.c_void_p()
    assert lib.css_pq_create(48, pq.codebooks.ctypes.data, 0, ctypes.byref(out)) == nat.CSS_ERR_INVALID
    assert "d=48 must be a multiple of 32" in nat.last_error()
    assert lib.css_pq_create(32, pq.codebooks.ctypes.data, 0, None) == nat.CSS_ERR_INVALID and "out is NULL" in nat.last_error()
