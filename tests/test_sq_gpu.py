"""GPU: the scalar-quantized store (css_sq_*, kernels in csrc/css_sq.h) against the numpy restatement of sq.py.
Everything is integers or single correctly rounded operations: every comparison is array_equal."""
import functools

import numpy as np
import pytest

from claude_semantic_search_amd.sq import IndexScalarQuantizer, ScalarQuantizer, search_numpy

pytestmark = pytest.mark.gpu

BITS = (4, 8)
DIMS = (32, 96, 768, 8192)   # one granule row, a partial last chunk, the usual (queries in registers), the maximum (in LDS)
N = 5000                     # 79 steps of 64 rows, the last one partial
KS = (1, 10, 128)


@functools.lru_cache(maxsize=None)
def quantizer(bits, d):
    """Even components on a power-of-two grid (half steps are exact), odd ones on an arbitrary one (the division rounds)."""
    rng = np.random.default_rng(10 * d + bits)
    vmin, step = rng.integers(-8, 8, d) * 0.25, 2.0 ** rng.integers(-3, 2, d)
    vmin[1::2], step[1::2] = rng.standard_normal(d // 2), rng.uniform(0.01, 1.0, d // 2)
    return ScalarQuantizer(d, bits, vmin, step)


@functools.lru_cache(maxsize=None)
def codes(bits, d, family):
    """N rows of codes, row 0 all L and row 1 all 0.  "ties": the levels {0, 1, L - 1, L}; "full": uniform."""
    L, rng = 2 ** bits - 1, np.random.default_rng(100 + d + bits)
    lv = rng.integers(0, L + 1, size=(N, d)) if family == "full" else np.array([0, 1, L - 1, L])[rng.integers(0, 4, size=(N, d))]
    lv[0], lv[1] = L, 0
    return (lv if bits == 8 else lv[:, 0::2] | lv[:, 1::2] << 4).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def store(bits, d, family):
    ix = IndexScalarQuantizer(quantizer(bits, d))
    ix.add_codes(codes(bits, d, family))
    return ix


@functools.lru_cache(maxsize=None)
def queries(bits, d, family):
    """(33 int8 queries, their scores).  "ties": components in {-1, 0, 1} against four levels, so ties straddle rank k;
    "full": the whole of int8, query 0 all -128 and query 1 all 127: at d = 8192 the scores reach the extremes."""
    rng = np.random.default_rng(7 if d == 32 else 200 + d)
    if family == "ties":
        q8 = rng.integers(-1, 2, size=(33, d), dtype=np.int8)
    else:
        q8 = rng.integers(-128, 128, size=(33, d), dtype=np.int8)
        q8[0], q8[1] = -128, 127
    s = quantizer(bits, d).scores_numpy(q8, codes(bits, d, family))
    if family == "ties" and d == 32:   # (conditions on the inputs: the kernel is not involved)
        t = -np.sort(-s, axis=1)
        assert all((t[:, k - 1] == t[:, k]).sum() > (8 if k >= 10 else 0) for k in KS)
    if family == "full":
        L = 2 ** bits - 1
        assert s[0, 0] == -128 * L * d and s[1, 0] == 127 * L * d and (s[0] <= 0).all() and s[0, 1] == 0
    s.setflags(write=False)
    return q8, s


@functools.lru_cache(maxsize=None)
def allow_mask():
    m = np.random.default_rng(7).random(N) < 0.4
    m[4990:] = True   # (rows of the partial last step among them)
    return m


@functools.lru_cache(maxsize=None)
def reference(bits, d, family, k, masked):
    return search_numpy(queries(bits, d, family)[1], k, allow_mask() if masked else None)


@pytest.mark.parametrize("n", (1, 63, 65, 1000))
@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("bits", BITS)
def test_codes(bits, d, n):
    """add of float rows (clamped below and above, on exact half steps, on a grid where the division rounds) gives
    encode_numpy's bytes, at once or in pieces; add_codes / get_codes round-trips; reconstruct_n is decode_numpy."""
    import torch

    sq, rng = quantizer(bits, d), np.random.default_rng(n + d)
    x = (sq.vmin + sq.step * (rng.integers(-4, 2 * sq.L + 8, size=(n, d)) / 2)).astype(np.float32)
    x[:, 1::2] = (sq.vmin + sq.step * rng.uniform(-2, sq.L + 2, size=(n, d)))[:, 1::2]
    x[0, :3] = (-0.0, sq.vmin[1] - 1e30, sq.vmin[2] + 1e30)
    want = sq.encode_numpy(x)
    lv = sq.levels(want)
    assert lv.min() == 0 and lv.max() == sq.L and want.shape == (n, d * bits // 8)
    cuts = sorted({0, n // 3, min(n, 64), n})
    with IndexScalarQuantizer(sq) as a, IndexScalarQuantizer(sq) as b, IndexScalarQuantizer(sq) as c:
        a.add(x)
        for r0, r1 in zip(cuts, cuts[1:]):   # (host and device pieces in turn)
            b.add(x[r0:r1]) if r0 % 2 else b.add_dev(torch.from_numpy(x[r0:r1]).cuda())
            c.add_codes(want[r0:r1])
        for ix in (a, b, c):
            assert ix.ntotal == n and np.array_equal(ix.get_codes(), want)
        assert np.array_equal(c.get_codes(n // 2, n - n // 2), want[n // 2:])
        assert np.array_equal(a.reconstruct_n().view(np.int32), sq.decode_numpy(want).view(np.int32))
        assert np.array_equal(b.reconstruct_n(n - 1, 1), sq.decode_numpy(want[n - 1:]))


@pytest.mark.parametrize("masked", (False, True))
@pytest.mark.parametrize("waves", (0, 1, 3))   # a wave walks 1, 79 or 27 steps: the merge, the threshold and the insert path
@pytest.mark.parametrize("family", ("ties", "full"))
@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("bits", BITS)
def test_search_is_the_restatement(bits, d, family, waves, masked):
    ix, q8 = store(bits, d, family), queries(bits, d, family)[0]
    ix.set_waves(waves)
    try:
        for k in KS:
            Dr, Ir = reference(bits, d, family, k, masked)
            for nq in (1, 3, 16, 17, 33):
                D, I = ix.search_i8(q8[:nq], k, allow_mask() if masked else None)
                assert D.dtype == np.int32 and I.dtype == np.int64 and ix.last_passes == -(-nq // 16)
                assert np.array_equal(I, Ir[:nq]) and np.array_equal(D, Dr[:nq]), (k, nq)
    finally:
        ix.set_waves(0)


@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("bits", BITS)
def test_forms_agree(bits, d):
    """The float form is search_i8 of quantize_queries_numpy's int8 (a zero query and one whose folded maximum is
    denormal among Gaussian ones); the _dev forms give the bytes of the host forms."""
    import torch

    ix, rows, sq = store(bits, d, "full"), codes(bits, d, "full"), quantizer(bits, d)
    q = np.random.default_rng(300 + d).standard_normal((19, d)).astype(np.float32)
    q[3] = 0
    q[5] = 0
    q[5, ::7] = 1e-39
    q8 = sq.quantize_queries_numpy(q)[0]
    assert not q8[3].any() and not q8[5].any() and (np.abs(q8).max(axis=1)[[0, 18]] == 127).all()
    for mask in (None, allow_mask()):
        Dr, Ir = search_numpy(sq.scores_numpy(q8, rows), 10, mask)
        for got in (ix.search_i8(q8, 10, mask), ix.search(q, 10, mask), ix.search_dev(torch.from_numpy(q).cuda(), 10, mask),
                    ix.search_i8_dev(torch.from_numpy(q8).cuda(), 10, mask)):
            Dg, Ig = (np.asarray(t.cpu() if hasattr(t, "cpu") else t) for t in got)
            assert Dg.dtype == np.int32 and np.array_equal(Dg, Dr) and np.array_equal(Ig, Ir)


@pytest.mark.parametrize("n", (1, 63, 65, 257))
@pytest.mark.parametrize("bits", BITS)
def test_padding(bits, n):
    """An empty store answers with padding.  k = 128 under the all -128 query, where every real row scores at most 0
    and a zero code in the last tile's tail would beat them: the n real rows, then INT32_MIN / -1."""
    sq, rng = quantizer(bits, 96), np.random.default_rng(n)
    rows = rng.integers(0, 256, size=(n, sq.code_size), dtype=np.uint8)
    q8 = np.full((1, 96), -128, dtype=np.int8)
    with IndexScalarQuantizer(sq) as ix:
        D, I = ix.search_i8(q8, 5)
        assert (D == -2 ** 31).all() and (I == -1).all() and ix.last_passes == 0
        ix.add_codes(rows)
        for mask in (None, np.arange(n) % 3 == 0):
            D, I = ix.search_i8(q8, 128, mask)
            Dr, Ir = search_numpy(sq.scores_numpy(q8, rows), 128, mask)
            assert np.array_equal(I, Ir) and np.array_equal(D, Dr)
            real = min(128, n if mask is None else -(-n // 3))
            assert (I[0, :real] >= 0).all() and (I[0, real:] == -1).all() and (D[0, real:] == -2 ** 31).all()
