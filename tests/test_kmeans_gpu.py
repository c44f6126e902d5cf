"""GPU: one Lloyd step on the HIP index (``css_index_kmeans_step``), ``reconstruct_batch``, ``IndexFlat.kmeans``,
``Kmeans`` and the sharded k-means, against the float64 statement of ``kmeans_fakes`` and the integer statements of
``flat_index``.

Exact data: rows and centroids with entries that are multiples of 1/8 in [-2, 2].  Every product is a multiple of 1/64
and every partial sum over up to 768 columns stays below 2^24 / 64, so dot products, squared norms, keys (multiples of
1/128) and distances are exact in fp32 WHATEVER the summation order: assignment, distance, sums, counts and objective
are compared bit for bit.  Gaussian data: the tolerance of the issue, ``tol_r = 2 d u (|x||c| + |c|^2 / 2)`` with
``u = 2^-24`` and ``c`` the row's centroid -- twice the textbook bound of a length-d fp32 dot product, because the
rounding inside a two-product matrix-core step is not documented."""
import os
import socket

import numpy as np
import pytest

from kmeans_fakes import GAUSS_CASES, FakeKmeansIndex, assign64, gaussian_case, keys64, planted

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
NCS = (2, 5, 128, 129, 300)


def _fi():
    from claude_semantic_search_amd import flat_index as fi
    return fi


def _exact(n, d, nc, seed):
    """Rows and centroids in multiples of 1/8 in [-2, 2]; half of the centroids are copies of rows, and centroids 1,
    nc - 1 duplicate centroids 0 and nc / 2, so that exact ties exist in the first, a middle and the last tile."""
    rng = np.random.default_rng(seed)
    x = (rng.integers(-16, 17, size=(n, d)) / 8.0).astype(np.float32)
    c = (rng.integers(-16, 17, size=(nc, d)) / 8.0).astype(np.float32)
    c[::2] = x[rng.integers(0, n, size=c[::2].shape[0])]
    c[1] = c[0]
    c[nc - 1] = c[nc // 2]
    return x, c


def _mask(n):
    """Whole 32-row words and single rows cleared."""
    allow = np.ones(n, bool)
    allow[32:64] = False
    allow[1024:1056] = False
    allow[::7] = False
    allow[n - 1:] = n % 2 == 0
    return allow


def _check_integers(fi, x, st, nc, ix):
    """sums, counts and objective are the numpy statements of the step's OWN assign and dist, bit for bit, under the
    shift ``kmeans_shift`` predicts."""
    s, e, t = fi.kmeans_shift(ix.bounds()["max_norm2"], x.shape[0])
    assert (st.fx_shift, st.obj_shift) == (s, t)
    sums, counts = fi.fixed_point_sums(x, st.assign, nc, s)
    assert np.array_equal(st.counts, counts)
    assert np.array_equal(st.sums, sums)
    assert st.obj == fi.fixed_point_objective(st.dist, st.assign, t)
    assert st.sums.dtype == np.int64 and st.counts.dtype == np.int64


@pytest.mark.parametrize("n", (1, 127, 1037, 5000))
@pytest.mark.parametrize("d", (768, 100))
def test_step_on_exact_data_is_the_float64_statement_bit_for_bit(d, n):
    fi = _fi()
    ix = fi.IndexFlatL2(d)
    x, _ = _exact(n, d, 2, 1000 + n + d)
    ix.add(x)
    for nc in NCS:
        _, c = _exact(n, d, nc, 7 * nc + n)
        c[::2] = x[np.random.default_rng(nc).integers(0, n, size=c[::2].shape[0])]
        c[1], c[nc - 1] = c[0], c[nc // 2]
        for allow in (None, _mask(n)):
            st = ix.kmeans_step(c, allow=allow, want_assign=True, want_dist=True)
            a, dist, _ = assign64(x, c, allow)
            assert np.array_equal(st.assign, a), (nc, allow is not None)
            assert st.dist.tobytes() == dist.tobytes(), (nc, allow is not None)
            _check_integers(fi, x, st, nc, ix)
            assert int(st.counts.sum()) == (n if allow is None else int(allow.sum()))
            assert not st.counts[1] and (nc == 2 or not st.counts[nc - 1] or nc // 2 == nc - 1)   # ties went to the lower index
    if n == 5000:
        big = ix.kmeans_step(np.stack([c[0], c[0]]), want_assign=True)
        assert big.counts.tolist() == [5000, 0]          # one cluster of five 1024-member segments
        assert np.array_equal(big.sums[0], fi.fixed_point_sums(x, big.assign, 2, big.fx_shift)[0][0])
    ix.close()


@pytest.mark.parametrize("d, scale, seed", GAUSS_CASES)
def test_step_on_gaussian_data_is_within_the_rounding_tolerance(d, scale, seed):
    fi = _fi()
    x, c = gaussian_case(d, scale, seed)
    n, nc = x.shape[0], c.shape[0]
    for metric, mode in ((1, None), (0, "exact_fp32"), (0, "coarse")):    # neither the metric nor the search mode plays a part
        ix = fi.IndexFlat(d, metric)
        if mode:
            ix.set_search_mode(mode)
        ix.add(x)
        st = ix.kmeans_step(c, want_assign=True, want_dist=True)
        if metric == 1:
            first = st
        else:
            assert st.assign.tobytes() == first.assign.tobytes() and st.dist.tobytes() == first.dist.tobytes()
            assert st.sums.tobytes() == first.sums.tobytes() and st.obj == first.obj
        ix.close()
    st = first
    key = keys64(x, c)
    a64 = key.argmax(axis=1)
    xn = np.linalg.norm(x.astype(np.float64), axis=1)
    cn = np.linalg.norm(c.astype(np.float64), axis=1)[st.assign]
    tol = 2.0 * d * U * (xn * cn + 0.5 * cn * cn)
    got = key[np.arange(n), st.assign]
    short = key.max(axis=1) - got
    dist64 = np.maximum(0.0, xn * xn - 2.0 * got)
    derr = np.abs(st.dist.astype(np.float64) - dist64)
    differ = int((st.assign != a64).sum())
    print(f"d={d} scale={scale}: {differ} of {n} rows differ from the float64 argmax; worst key shortfall / (2 tol) = "
          f"{float((short / (2 * tol)).max()):.3g}; worst dist error / bound = "
          f"{float((derr / (2 * tol + 4 * U * xn * xn)).max()):.3g}")
    assert (st.assign >= 0).all() and (st.assign < nc).all()
    assert (short <= 2.0 * tol).all()
    assert (derr <= 2.0 * tol + 4.0 * U * xn * xn).all()
    assert differ <= n // 100
    ix = fi.IndexFlatL2(d)
    ix.add(x)
    _check_integers(fi, x, st, nc, ix)
    ix.close()


def test_the_same_call_gives_the_same_bytes():
    fi = _fi()
    x, c = gaussian_case(768, 1.0, 77, n=5000, nc=300)
    ix = fi.IndexFlatIP(768)
    ix.add(x)
    allow = _mask(5000)

    def run():
        st = ix.kmeans_step(c, allow=allow, want_assign=True, want_dist=True)
        return b"".join(a.tobytes() for a in (st.sums, st.counts, st.assign, st.dist)) + repr((st.obj, st.fx_shift, st.obj_shift)).encode()

    one = run()
    assert run() == one
    ix.search(x[:40], 10)                                # an unrelated search in between (it shares the workspaces)
    ix.search(x[:3], 5, allow=~allow)
    assert run() == one
    ix.close()


def test_the_shift_follows_the_largest_row_and_an_imposed_shift_is_checked():
    fi = _fi()
    from claude_semantic_search_amd import _native as nat

    x, c = _exact(1037, 100, 5, 5)
    ix = fi.IndexFlatL2(100)
    ix.add(x)
    before = ix.kmeans_step(c)
    ix.add(x[:1] * np.float32(1000.0))                   # one long row
    xx = np.concatenate([x, x[:1] * np.float32(1000.0)])
    st = ix.kmeans_step(c, want_assign=True, want_dist=True)
    s, e, t = fi.kmeans_shift(ix.bounds()["max_norm2"], 1038)
    assert e == fi.kmeans_shift(float((xx[-1].astype(np.float64) ** 2).sum()), 1038)[1]
    assert (st.fx_shift, st.obj_shift) == (s, t) and st.fx_shift <= before.fx_shift - 9      # 1000 > 2^9
    _check_integers(fi, xx, st, 5, ix)
    # an imposed shift: at the safe value and below it is used as given; one above is refused, with the safe value named
    low = ix.kmeans_step(c, fx_shift=s - 3, want_assign=True)
    assert low.fx_shift == s - 3 and low.obj_shift == t - 3
    assert np.array_equal(low.sums, fi.fixed_point_sums(xx, low.assign, 5, s - 3)[0])
    assert ix.kmeans_step(c, fx_shift=s).sums.tobytes() == st.sums.tobytes()
    with pytest.raises(nat.CssError, match=rf"largest safe value is {s}\b") as err:
        ix.kmeans_step(c, fx_shift=s + 1)
    assert err.value.code == nat.CSS_ERR_INVALID
    again = ix.kmeans_step(c, want_assign=True, want_dist=True)      # the index still works
    assert again.sums.tobytes() == st.sums.tobytes() and again.obj == st.obj
    D, I = ix.search(x[:2], 1)
    assert I[:, 0].tolist() == [0, 1]
    ix.close()


def test_arguments_are_checked_before_anything_runs():
    fi = _fi()
    from claude_semantic_search_amd import _native as nat

    x, c = _exact(127, 100, 5, 9)
    ix = fi.IndexFlatL2(100)
    ix.add(x)
    for nc in (1, 4097):
        with pytest.raises(ValueError, match="outside"):
            ix.kmeans_step(np.zeros((nc, 100), np.float32))
        buf = np.zeros((nc, 100), np.float32)
        out = np.zeros(nc * 100 + nc + 1, np.int64)
        rc = nat.lib().css_index_kmeans_step(ix._handle(), buf.ctypes.data, nc, -1, None, out.ctypes.data, out.ctypes.data,
                                             out.ctypes.data, None, None, None, None)
        assert rc == nat.CSS_ERR_INVALID and f"nc={nc}" in nat.last_error()
    for bad, word in ((np.nan, "NaN"), (np.inf, "infinite")):
        cc = c.copy()
        cc[3, 17] = bad
        with pytest.raises(nat.CssError, match=rf"centroid 3 has a {word}"):
            ix.kmeans_step(cc)
    with pytest.raises(ValueError):
        ix.kmeans_step(np.zeros((5, 99), np.float32))
    with pytest.raises(ValueError):
        ix.kmeans_step(c, allow=np.ones(126, bool))
    assert int(ix.kmeans_step(c).counts.sum()) == 127
    ix.close()


def test_reconstruct_batch():
    fi = _fi()
    from claude_semantic_search_amd import _native as nat

    for d in (768, 100, 10):                              # (10: rows that are no multiple of 16 bytes)
        x = np.random.default_rng(d).standard_normal((300, d)).astype(np.float32)
        ix = fi.IndexFlatIP(d)
        ix.add(x)
        ids = np.array([299, 0, 5, 5, 128, 5, 299], np.int64)
        assert ix.reconstruct_batch(ids).tobytes() == x[ids].tobytes()
        assert ix.reconstruct_batch([]).shape == (0, d)
        ix.set_id_base(1000)
        assert ix.reconstruct_batch(ids + 1000).tobytes() == x[ids].tobytes()
        for bad in (999, 1300, -1):
            with pytest.raises(nat.CssError, match=rf"id {bad} "):
                ix.reconstruct_batch([1000, bad])
        with pytest.raises(ValueError):
            ix.reconstruct_batch([0.5])
        assert ix.reconstruct_batch([1299]).tobytes() == x[299:].tobytes()   # the index still works
        ix.close()


def test_the_step_follows_the_rows_through_remove_add_and_reset():
    fi = _fi()
    d, nc = 100, 5
    x, c = _exact(1037, d, nc, 31)
    ix = fi.IndexFlatL2(d)
    empty = ix.kmeans_step(c, want_assign=True, want_dist=True)
    assert not empty.sums.any() and not empty.counts.any() and empty.obj == 0
    assert empty.assign.shape == (0,) and empty.dist.shape == (0,)
    assert (empty.fx_shift, empty.obj_shift) == fi.kmeans_shift(0.0, 0)[::2]

    def check(rows):
        st = ix.kmeans_step(c, want_assign=True, want_dist=True)
        a, dist, _ = assign64(rows, c)
        assert np.array_equal(st.assign, a) and st.dist.tobytes() == dist.tobytes()
        _check_integers(fi, rows, st, nc, ix)

    ix.add(x[:300])
    check(x[:300])
    gone = np.arange(0, 300, 3)
    assert ix.remove_ids(gone) == 100
    kept = np.delete(x[:300], gone, axis=0)
    check(kept)
    ix.add(x[300:])                                      # grows the capacity: the rows move
    check(np.concatenate([kept, x[300:]]))
    ix.reset()
    assert not ix.kmeans_step(c).counts.any()
    ix.add(x[:127])
    check(x[:127])
    ix.close()


def _good_seed(fi, lab, nc):
    return next(sd for sd in range(1 << 14) if len(set(lab[fi.kmeans_init_ids(np.arange(lab.shape[0]), nc, sd)].tolist())) == nc)


def test_kmeans_on_planted_clusters_equals_the_double_and_kmeans_class():
    fi = _fi()
    x, lab, C = planted(4096, 768, 8, seed=12)
    seed = _good_seed(fi, lab, 8)                        # (a start with one row of every cluster: see test_kmeans_host)
    fake = FakeKmeansIndex(768, 1)
    fake.add(x)
    ref = fake.kmeans(8, niter=10, seed=seed)
    ix = fi.IndexFlatL2(768)
    ix.add(x)
    res = ix.kmeans(8, niter=10, seed=seed)
    assert np.array_equal(res.assign, ref.assign) and np.array_equal(res.sizes, ref.sizes)
    assert res.centroids.tobytes() == ref.centroids.tobytes() and res.iterations == ref.iterations < 10
    assert len(set(zip(res.assign.tolist(), lab.tolist()))) == 8          # the planted partition
    for i in range(1, len(res.obj)):
        if not res.splits[i - 1]:
            assert res.obj[i] <= res.obj[i - 1] * (1.0 + 1e-6)
    n2 = float((x.astype(np.float64) ** 2).sum(axis=1).max())            # centroids are means: no longer than the rows
    bound = 2.0 * (2.0 * 768 * U * 1.5 * n2) + 4.0 * U * n2               # the distance bound of the Gaussian test
    assert np.abs(res.dist.astype(np.float64) - ref.dist).max() <= bound
    # the same call, the same bytes; a mask leaves rows out; a training subset still assigns all
    again = ix.kmeans(8, niter=10, seed=seed)
    assert again.centroids.tobytes() == res.centroids.tobytes() and again.assign.tobytes() == res.assign.tobytes()
    allow = (np.arange(4096) % 5) != 2
    part = ix.kmeans(8, niter=4, init=res.centroids, allow=allow)
    assert (part.assign[~allow] == -1).all() and np.array_equal(part.assign[allow], res.assign[allow])
    sub = ix.kmeans(8, niter=4, init=res.centroids, max_points_per_centroid=64)
    assert np.array_equal(sub.assign, res.assign) and int(sub.sizes.sum()) == 4096
    with pytest.raises(ValueError, match="allowed rows"):
        ix.kmeans(8, allow=np.arange(4096) < 5)
    ix.close()
    # spherical (the default of an inner-product index): unit centroids
    ip = fi.IndexFlatIP(768)
    ip.add(x, normalize=True)
    sph = ip.kmeans(8, niter=6, seed=seed)
    assert np.abs(np.linalg.norm(sph.centroids.astype(np.float64), axis=1) - 1.0).max() <= 1e-6
    assert len(set(zip(sph.assign.tolist(), lab.tolist()))) == 8
    ip.close()
    # faiss-shaped
    km = fi.Kmeans(768, 8, niter=10, seed=seed)
    last = km.train(x)
    assert km.centroids.tobytes() == res.centroids.tobytes() and last == km.obj[-1] == res.obj[-1]
    D, I = km.assign(x)
    assert np.array_equal(I, res.assign.astype(np.int64))
    assert np.abs(D.astype(np.float64) - res.dist).max() <= 2.0 * bound     # (two fp32 evaluations of one distance)
    assert km.index.ntotal == 8
    km.index.close()


# ----------------------------------------------------------------------------- two ranks on one GPU
def _sharded_data():
    return gaussian_case(768, 1.0, 55, n=3001, nc=16)


def _rank(rank, world, port, out_dir):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import torch
    import torch.distributed as dist

    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from claude_semantic_search_amd.sharded import ShardedFlatIndex

        torch.cuda.set_device(0)
        x, c = _sharded_data()
        sh = ShardedFlatIndex(768, 0, device_index=0)
        sh.add_global(x[:2000])
        sh.add_routed(x[2000:2300] * np.float32(3.0))    # longer rows on ONE shard: the global maximum sets the shift
        sh.add_global(x[2300:])
        res = sh.kmeans(16, niter=5, seed=3)
        rows = sh.reconstruct_batch(np.array([0, 3000, 2100, 2100, 1500], np.int64))
        np.savez(os.path.join(out_dir, f"k{rank}.npz"), c=res.centroids, sizes=res.sizes, obj=np.array(res.obj),
                 a=res.assign, d=res.dist, mine=sh.local_rows_of(np.arange(3001)), rows=rows)
    finally:
        dist.destroy_process_group()


def test_two_ranks_on_one_gpu_equal_one_index_bit_for_bit(tmp_path):
    import torch.multiprocessing as mp

    fi = _fi()
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    mp.spawn(_rank, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    x, c = _sharded_data()
    x[2000:2300] *= np.float32(3.0)
    ix = fi.IndexFlatIP(768)
    ix.add(x)
    ref = ix.kmeans(16, niter=5, seed=3)
    ix.close()
    sizes = []
    for r in range(2):
        g = np.load(tmp_path / f"k{r}.npz")
        assert g["c"].tobytes() == ref.centroids.tobytes(), r
        assert np.array_equal(g["sizes"], ref.sizes) and np.array_equal(g["obj"], np.array(ref.obj)), r
        assert np.array_equal(g["a"], ref.assign[g["mine"]]) and g["d"].tobytes() == ref.dist[g["mine"]].tobytes(), r
        assert g["rows"].tobytes() == x[[0, 3000, 2100, 2100, 1500]].tobytes(), r
        sizes.append(g["mine"].shape[0])
    assert sum(sizes) == 3001 and min(sizes) > 1000
