"""GPU: the binary row store (css_bin_*, csrc/css_binary.h) against the numpy restatement of binary.py.  Everything is
integers: every comparison is array_equal, with no tolerance and no tie window."""
import ctypes
import functools

import numpy as np
import pytest

from claude_semantic_search_amd import _native as nat
from claude_semantic_search_amd.binary import IndexBinaryFlat, binarize_numpy, hamming_numpy, search_numpy

pytestmark = pytest.mark.gpu

DIMS = (32, 96, 768, 8192)   # one word, an odd number of words (half a 64-float chunk), the usual, the maximum
N = 5000                     # 20 steps of 256 rows, the last one partial
KS = (1, 10, 128)


def float_rows(n, d, seed):
    """Gaussian rows with 0.0, -0.0 and denormals of both signs strewn in."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, d)).astype(np.float32)
    special = np.array([0.0, -0.0, 1e-45, -1e-45, 1e-39, -1e-39], dtype=np.float32)
    hit = rng.random((n, d)) < 0.3
    x[hit] = special[rng.integers(0, special.size, size=int(hit.sum()))]
    return x


@functools.lru_cache(maxsize=None)
def store(d):
    """(store of N uniform random codes, 33 query codes, their distances): built once per d."""
    rng = np.random.default_rng(100 + d)
    rows = rng.integers(0, 256, size=(N, d // 8), dtype=np.uint8)
    q = rng.integers(0, 256, size=(33, d // 8), dtype=np.uint8)
    ix = IndexBinaryFlat(d)
    ix.add(rows)
    h = hamming_numpy(q, rows)
    if d == 32:   # 33 possible distances among 5000 rows: ties straddle rank k, at k >= 10 in most queries
        s = np.sort(h, axis=1)
        assert all((s[:, k - 1] == s[:, k]).sum() > (16 if k >= 10 else 0) for k in KS)
    h.setflags(write=False)
    return ix, q, h


@functools.lru_cache(maxsize=None)
def allow_mask():
    m = np.random.default_rng(7).random(N) < 0.4
    m[4990:] = True   # (rows of the partial last step among them)
    return m


@functools.lru_cache(maxsize=None)
def reference(d, k, masked):
    return search_numpy(store(d)[2], k, allow_mask() if masked else None)


@pytest.mark.parametrize("n", (1, 63, 65, 1000))
@pytest.mark.parametrize("d", DIMS)
def test_codes_of_float_rows(d, n):
    x = float_rows(n, d, d + n)
    with IndexBinaryFlat(d) as ix:
        ix.add_float(x)
        assert ix.ntotal == n and np.array_equal(ix.get_codes(), binarize_numpy(x))


def test_growth_and_round_trip():
    """The second add outgrows the planes of the first; add(get_codes()) stores the same rows again."""
    import torch

    x = float_rows(1100, 96, 5)
    with IndexBinaryFlat(96) as ix:
        ix.add_float(x[:100])
        ix.add_dev(torch.from_numpy(x[100:]).cuda())
        want = binarize_numpy(x)
        assert np.array_equal(ix.get_codes(), want) and np.array_equal(ix.get_codes(99, 3), want[99:102])
        ix.add(ix.get_codes())
        assert ix.ntotal == 2200 and np.array_equal(ix.get_codes(1100), want)


@pytest.mark.parametrize("masked", (False, True))
@pytest.mark.parametrize("waves", (0, 1, 3))   # a wave walks 1, 20 or 7 steps: the merge, the threshold and the insert path
@pytest.mark.parametrize("d", DIMS)
def test_search_is_the_restatement(d, waves, masked):
    ix, q, _ = store(d)
    ix.set_waves(waves)
    try:
        for k in KS:
            Dr, Ir = reference(d, k, masked)
            for nq in (1, 3, 16, 17, 33):
                D, I = ix.search(q[:nq], k, allow_mask() if masked else None)
                assert D.dtype == np.int32 and I.dtype == np.int64 and ix.last_passes == -(-nq // 16)
                assert np.array_equal(I, Ir[:nq]) and np.array_equal(D, Dr[:nq]), (k, nq)
    finally:
        ix.set_waves(0)


@pytest.mark.parametrize("waves", (0, 2))
@pytest.mark.parametrize("n", (1, 255, 257))
def test_padding_and_identical_rows(n, waves):
    """k = 128 with n = 1 rows, or with the 1 + n // 3 rows a mask leaves, pads; rows that all equal the query come back
    as ids 0 .. k - 1 at distance 0."""
    rng = np.random.default_rng(n)
    rows, q = rng.integers(0, 256, size=(n, 12), dtype=np.uint8), rng.integers(0, 256, size=(3, 12), dtype=np.uint8)
    allow = np.arange(n) % 3 == 0
    with IndexBinaryFlat(96) as ix:
        D, I = ix.search(q, 5)
        assert (D == 2 ** 31 - 1).all() and (I == -1).all() and ix.last_passes == 0
        ix.add(rows)
        ix.set_waves(waves)
        for mask in (None, allow):
            D, I = ix.search(q, 128, mask)
            Dr, Ir = search_numpy(hamming_numpy(q, rows), 128, mask)
            assert np.array_equal(I, Ir) and np.array_equal(D, Dr)
            assert (I[:, -1] == -1).all() or (mask is None and n > 128)
    with IndexBinaryFlat(96) as ix:
        ix.add(np.repeat(q[:1], n + 300, axis=0))
        ix.set_waves(waves)
        D, I = ix.search(q[:1], 128)
        assert not D.any() and I.tolist() == [list(range(128))]


def test_forms_agree():
    """search_float is search of the binarized queries; the _dev forms give the bytes of the host forms; a query alone
    gets its row of a batch of 17."""
    import torch

    x, qf = float_rows(N, 768, 1), float_rows(17, 768, 2)
    qc = binarize_numpy(qf)
    with IndexBinaryFlat(768) as ix:
        ix.add_float(x)
        for mask in (None, allow_mask()):
            D, I = ix.search(qc, 10, mask)
            Dr, Ir = search_numpy(hamming_numpy(qc, binarize_numpy(x)), 10, mask)
            assert np.array_equal(D, Dr) and np.array_equal(I, Ir)
            for got in (ix.search_float(qf, 10, mask), ix.search_dev(torch.from_numpy(qf).cuda(), 10, mask),
                        ix.search_codes_dev(torch.from_numpy(qc).cuda(), 10, mask)):
                Dg, Ig = (np.asarray(t.cpu() if hasattr(t, "cpu") else t) for t in got)
                assert Dg.dtype == np.int32 and np.array_equal(Dg, D) and np.array_equal(Ig, I)
            D1, I1 = ix.search(qc[16:], 10, mask)
            assert np.array_equal(D1, D[16:]) and np.array_equal(I1, I[16:])


def test_library_refusals():
    """The C ABI checks its arguments before anything is enqueued: k, and a NaN named by row and component."""
    lib, h = nat.lib(), ctypes.c_void_p()
    nat.check(lib.css_bin_create(64, 0, ctypes.byref(h)))
    x = np.zeros((3, 64), dtype=np.float32)
    D, I = np.zeros((3, 200), dtype=np.int32), np.zeros((3, 200), dtype=np.int64)
    for k in (0, 129):
        assert lib.css_bin_search(h, x.ctypes.data, 3, k, None, D.ctypes.data, I.ctypes.data) == nat.CSS_ERR_INVALID
        assert f"k={k} outside [1, 128]" in nat.last_error()
    x[2, 5] = np.nan
    assert lib.css_bin_add(h, x.ctypes.data, 3) == nat.CSS_ERR_INVALID and "component 5 of row 2 is NaN" in nat.last_error()
    assert lib.css_bin_search(h, x.ctypes.data, 3, 1, None, D.ctypes.data, I.ctypes.data) == nat.CSS_ERR_INVALID
    assert "component 5 of query 2 is NaN" in nat.last_error()
    assert lib.css_bin_set_waves(h, 1 << 20) == nat.CSS_ERR_INVALID
    n = ctypes.c_int64(-1)
    nat.check(lib.css_bin_ntotal(h, ctypes.byref(n)))
    assert n.value == 0
    nat.check(lib.css_bin_free(h))
