"""GPU: ``css_index_gram`` and ``css_index_transform`` on the HIP index, ``IndexFlat.pca``, ``PCAMatrix``,
``HybridStorage.map`` and the sharded PCA, against the integer statement ``flat_index.fixed_point_gram`` and the float64
statement of ``pca_fakes``.

The Gram matrix, the column sums and the count are compared with ``array_equal``: they are exact integers, so there is
no tolerance.  The transform is compared with the worst-case bound of an fp32 dot product of ``dpad`` terms plus one
addition summed in ANY order, ``|y - y64| <= gamma (sum_j |x_j A_cj| + |b_c|)`` with ``gamma = k u / (1 - k u)``,
``k = dpad + 1``, ``u = 2^-24``: a derivation, not a measurement.

One case of the issue cannot exist as written: rows of d = 64 with EVERY component ``+-2^e (1 - 2^-20)`` have
``||x||^2`` just below ``64 * 2^(2e)``, so the exponent the shift rule derives from the norm is ``e + 3`` and the
quantised entries stay near ``2^17``: no partial sum comes near ``2^53``.  The case is kept as written (it crosses the
fold boundary with every entry of the matrix at the largest magnitude such rows allow), and a second one is added that
DOES reach ``2^53``: rows whose first column is ``+-2 (1 - 2^-20)`` and whose other columns are tiny, so that ``e = 1``,
``p = 19``, ``q = 2^20 - 1``, the fp64 partial sum of ``gram[0][0]`` over 8192 rows is ``2^53 - 2^34 + 2^13`` and the
total over ``8192 + 5`` rows is an odd number above ``2^53`` that no double holds.

The fold runs only in a block that owns more than 8192 rows, and the library's strip rule gives small inputs 512-row
strips (on 256 CUs a strip passes 8192 rows only beyond ~400 k rows at d = 768, never below 8 M rows at d <= 128).  So
every Gram case is run under the rule AND under ``set_gram_rows`` values that put all rows into ONE block (folds at
8192, and at 16384 where the case has the rows, then a tail), exactly 8192 rows per block (the fold is the last thing
a block does), and 16 rows per block (one chunk); all must give the same integers."""
import os
import socket

import numpy as np
import pytest

from kmeans_fakes import FakeKmeansIndex
from pca_fakes import FakePcaIndex, planted_pca, transform64

pytestmark = pytest.mark.gpu

U = 2.0 ** -24


def _fi():
    from claude_semantic_search_amd import flat_index as fi
    return fi


def _unit(n, d, seed):
    x = np.random.default_rng(seed).standard_normal((n, d))
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


def _rows(kind, n, d, seed):
    if kind == "unit":
        return _unit(n, d, seed)
    if kind == "norm3.7":
        return (_unit(n, d, seed).astype(np.float64) * 3.7).astype(np.float32)
    rng = np.random.default_rng(seed)
    if kind == "extreme":                                        # every component +-2^0 (1 - 2^-20)
        return (rng.choice([-1.0, 1.0], size=(n, d)) * (1.0 - 2.0 ** -20)).astype(np.float32)
    assert kind == "column"                                      # column 0 at +-2 (1 - 2^-20), the rest tiny
    x = rng.standard_normal((n, d)) * 1e-4
    x[:, 0] = rng.choice([-1.0, 1.0], size=n) * 2.0 * (1.0 - 2.0 ** -20)
    return x.astype(np.float32)


def _check_gram(fi, ix, x, allow=None, fx_shift=None):
    """The device's integers are those of ``fixed_point_gram`` under the shift ``pca_shift`` predicts; returns them."""
    n = x.shape[0]
    own = fi.pca_shift(ix.bounds()["max_norm2"] if n else 0.0, n)[0]
    g = ix.gram(allow=allow, fx_shift=fx_shift)
    assert g.shift == (own if fx_shift is None else fx_shift)
    gram, colsum, count = fi.fixed_point_gram(x, allow, g.shift)
    assert g.gram.dtype == np.int64 and g.gram.shape == (ix.d, ix.d) and g.colsum.shape == (ix.d,)
    assert g.count == count
    assert np.array_equal(g.colsum, colsum)
    assert np.array_equal(g.gram, gram)
    return g


GR_FOLD = 8192   # css_pca.h: rows between two folds of the fp64 accumulators

GRAM_CASES = (("unit", 768, 1000), ("unit", 72, 8192 * 2 + 77), ("unit", 72, 1), ("norm3.7", 72, 8270),
              ("extreme", 64, 8192 + 5), ("column", 64, 8192 + 5), ("unit", 100, 300))


@pytest.mark.parametrize("kind, d, n", GRAM_CASES)
def test_gram_is_the_integer_statement_exactly(kind, d, n):
    fi = _fi()
    x = _rows(kind, n, d, seed=n + d)
    ix = fi.IndexFlatIP(d)
    ix.add(x)
    g = _check_gram(fi, ix, x)
    p, e = fi.pca_shift(ix.bounds()["max_norm2"], n)
    if kind == "norm3.7":
        assert e == 2
    if kind == "column":
        assert (p, e) == (19, 1) and int(g.gram[0, 0]) == n * ((1 << 20) - 1) ** 2 > 1 << 53
    if kind == "extreme":
        assert int(g.gram[0, 0]) == n * int(fi._fixed(x[0, 0], p)) ** 2
    third = np.arange(n) % 3 == 0
    part = _check_gram(fi, ix, x, allow=third)
    assert part.count == int(third.sum())
    none = _check_gram(fi, ix, x, allow=np.zeros(n, bool))
    assert none.count == 0 and not none.gram.any() and not none.colsum.any()
    assert ix.gram().gram.tobytes() == g.gram.tobytes()          # (the masked calls in between left nothing behind)
    # other grids, the same integers: one block for all rows (n > 8192: it folds once or twice and then sums a tail),
    # blocks of exactly 8192 rows, and of one 16-row chunk (at most 65535 strips: d <= 128 only)
    for rows in (1 << 15, GR_FOLD) + ((16,) if d <= 128 else ()):
        ix.set_gram_rows(rows)
        _check_gram(fi, ix, x)
        _check_gram(fi, ix, x, allow=third)
    ix.set_gram_rows(0)
    assert ix.gram().gram.tobytes() == g.gram.tobytes()
    ix.close()


def test_gram_of_an_empty_index_and_through_remove_growth_and_reset():
    fi = _fi()
    d = 72
    x = _unit(3000, d, 17)
    ix = fi.IndexFlatL2(d)
    empty = ix.gram()
    assert empty.count == 0 and not empty.gram.any() and not empty.colsum.any() and empty.shift == fi.pca_shift(0.0, 0)[0]
    ix.reserve(400)
    ix.add(x[:300])
    _check_gram(fi, ix, x[:300])
    gone = np.arange(0, 300, 3)
    assert ix.remove_ids(gone) == 100
    kept = np.delete(x[:300], gone, axis=0)
    _check_gram(fi, ix, kept)
    ix.add(x[300:])                                              # grows past the reserved capacity: the rows move
    rows = np.concatenate([kept, x[300:]])
    _check_gram(fi, ix, rows)
    _check_gram(fi, ix, rows, allow=np.arange(rows.shape[0]) % 3 == 0)
    ix.reset()
    assert not ix.gram().gram.any()
    ix.add(x[:127])
    _check_gram(fi, ix, x[:127])
    ix.close()


def test_the_same_call_gives_the_same_bytes_and_an_imposed_shift_is_checked():
    fi = _fi()
    from claude_semantic_search_amd import _native as nat

    x = _unit(5000, 768, 23)
    ix = fi.IndexFlatIP(768)
    ix.add(x)
    allow = np.arange(5000) % 7 != 2

    def run():
        g = ix.gram(allow=allow)
        return g.gram.tobytes() + g.colsum.tobytes() + repr((g.count, g.shift)).encode()

    one = run()
    assert run() == one
    ix.search(x[:40], 10)                                        # an unrelated search in between (it shares the mask)
    ix.search(x[:3], 5, allow=~allow)
    assert run() == one
    p = fi.pca_shift(ix.bounds()["max_norm2"], 5000)[0]
    low = _check_gram(fi, ix, x, fx_shift=p - 4)
    assert low.shift == p - 4
    assert ix.gram(fx_shift=p).gram.tobytes() == ix.gram().gram.tobytes()
    with pytest.raises(nat.CssError, match=rf"largest safe value is {p}\b") as err:
        ix.gram(fx_shift=p + 1)
    assert err.value.code == nat.CSS_ERR_INVALID
    assert run() == one                                          # the index still works
    for rows in (1 << 20, 1008, 16):                             # any grid shape, the same bytes
        ix.set_gram_rows(rows)
        assert run() == one, rows
    with pytest.raises(nat.CssError, match="rows < 0"):
        ix.set_gram_rows(-1)
    ix.set_gram_rows(0)
    ix.add(x[:1] * np.float32(1000.0))                           # one long row: the shift follows it
    xx = np.concatenate([x, x[:1] * np.float32(1000.0)])
    g = _check_gram(fi, ix, xx)
    assert g.shift <= p - 9                                      # 1000 > 2^9
    ix.close()


def _gamma(dpad):
    k = dpad + 1
    return k * U / (1.0 - k * U)


@pytest.mark.parametrize("d", (72, 768))
def test_transform_is_within_the_fp32_accumulation_bound(d):
    fi = _fi()
    dpad = (d + 63) // 64 * 64
    rng = np.random.default_rng(d)
    x = (rng.standard_normal((300, d)) * 1.7).astype(np.float32)
    ix = fi.IndexFlatIP(d)
    ix.add(x)
    ix.set_search_mode("coarse")                                 # (the search mode plays no part)
    for m in (1, 2, 3, 128, 129, 256):
        A = rng.standard_normal((m, d)).astype(np.float32)
        b = rng.standard_normal(m).astype(np.float32)
        for bias in (b, None):
            y = ix.transform(A, bias, row0=5, n=131)
            y64, mag = transform64(x[5:136], A, bias)
            assert y.shape == (131, m) and y.dtype == np.float32
            ratio = float((np.abs(y.astype(np.float64) - y64) / (_gamma(dpad) * mag)).max())
            print(f"d={d} m={m} bias={bias is not None}: worst error / bound = {ratio:.3g}")
            assert ratio <= 1.0
        assert ix.transform(A, b, row0=7, n=0).shape == (0, m)
        whole = ix.transform(A, b)                               # every row, several row tiles
        y64, mag = transform64(x, A, b)
        assert whole.shape == (300, m) and (np.abs(whole.astype(np.float64) - y64) <= _gamma(dpad) * mag).all()
        assert whole[5:136].tobytes() == ix.transform(A, b, row0=5, n=131).tobytes()
    ix.close()


def test_transform_refuses_bad_arguments_before_anything_runs():
    fi = _fi()
    from claude_semantic_search_amd import _native as nat

    d = 72
    x = _unit(200, d, 3)
    ix = fi.IndexFlatL2(d)
    ix.add(x)
    A = np.ones((2, d), np.float32)
    for m in (0, 257):
        with pytest.raises(ValueError, match="outside"):
            ix.transform(np.zeros((m, d), np.float32))
        buf = np.zeros((max(m, 1), d), np.float32)
        out = np.zeros((200, max(m, 1)), np.float32)
        rc = nat.lib().css_index_transform(ix._handle(), buf.ctypes.data, None, m, 0, 200, out.ctypes.data)
        assert rc == nat.CSS_ERR_INVALID and f"m={m}" in nat.last_error()
    for bad, word in ((np.nan, "NaN"), (np.inf, "infinite")):
        AA = A.copy()
        AA[1, 17] = bad
        with pytest.raises(nat.CssError, match=rf"row 1 of A has a {word}") as err:
            ix.transform(AA)
        assert err.value.code == nat.CSS_ERR_INVALID
        with pytest.raises(nat.CssError, match=rf"entry 1 of b is {word}"):
            ix.transform(A, np.array([0.0, bad], np.float32))
    for row0, n in ((-1, 5), (190, 11), (201, 0)):
        with pytest.raises(ValueError, match="outside"):
            ix.transform(A, None, row0=row0, n=n)
    out = np.zeros((11, 2), np.float32)
    rc = nat.lib().css_index_transform(ix._handle(), A.ctypes.data, None, 2, 190, 11, out.ctypes.data)
    assert rc == nat.CSS_ERR_INVALID and "outside" in nat.last_error()
    with pytest.raises(ValueError):
        ix.transform(np.ones((2, d + 1), np.float32))
    with pytest.raises(ValueError):
        ix.transform(A, np.zeros(3, np.float32))
    y = ix.transform(A, None)                                    # the index still works
    assert np.abs(y[:, 0].astype(np.float64) - x.astype(np.float64).sum(axis=1)).max() <= _gamma(128) * np.abs(x).sum(axis=1).max()
    ix.close()


def test_the_kmeans_step_is_unchanged_by_the_shared_loop():
    """``k_kmeans_assign`` now runs the K loop it shares with ``k_transform_rows``: one step on exact data (entries
    that are multiples of 1/8, see test_kmeans_gpu) equals the float64 statement of ``FakeKmeansIndex`` bit for bit."""
    fi = _fi()
    rng = np.random.default_rng(41)
    for d, n, nc in ((768, 1037, 129), (100, 5000, 300)):
        x = (rng.integers(-16, 17, size=(n, d)) / 8.0).astype(np.float32)
        c = (rng.integers(-16, 17, size=(nc, d)) / 8.0).astype(np.float32)
        c[::2] = x[rng.integers(0, n, size=c[::2].shape[0])]
        c[1] = c[0]
        allow = np.arange(n) % 5 != 3
        fake = FakeKmeansIndex(d, 1)
        fake.add(x)
        ix = fi.IndexFlatL2(d)
        ix.add(x)
        for mask in (None, allow):
            st = ix.kmeans_step(c, allow=mask, want_assign=True, want_dist=True)
            ref = fake.kmeans_step(c, allow=mask, want_assign=True, want_dist=True)
            assert np.array_equal(st.assign, ref.assign) and st.dist.tobytes() == ref.dist.tobytes()
            assert np.array_equal(st.sums, ref.sums) and np.array_equal(st.counts, ref.counts)
            assert (st.obj, st.fx_shift, st.obj_shift) == (ref.obj, ref.fx_shift, ref.obj_shift)
        ix.close()


def test_pca_equals_pca_from_gram_of_the_doubles_integers_and_pcamatrix():
    fi = _fi()
    x, Uk = planted_pca(4000, 64, seed=3, mean=0.05)
    fake = FakePcaIndex(64, 1)
    fake.add(x)
    ix = fi.IndexFlatL2(64)
    ix.add(x)
    allow = np.arange(4000) % 4 != 1
    for kw in (dict(), dict(allow=allow), dict(whiten=True)):
        res, ref = ix.pca(3, **kw), fake.pca(3, **kw)
        assert all(np.asarray(a).tobytes() == np.asarray(b).tobytes() for a, b in zip(res, ref)), kw
    ref = fake.pca(3)
    assert np.linalg.svd(Uk @ ref.components.astype(np.float64).T, compute_uv=False).min() > 0.999
    with pytest.raises(ValueError, match="no rows"):
        ix.pca(2, allow=np.zeros(4000, bool))
    ix.close()
    # faiss-shaped
    pm = fi.PCAMatrix(64, 3)
    pm.train(x)
    assert pm.is_trained and pm.A.tobytes() == ref.components.tobytes() and pm.mean.tobytes() == ref.mean.tobytes()
    assert pm.b.tobytes() == fi.pca_offset(ref.components, ref.mean).tobytes()
    y = pm.apply(x)
    y64, mag = transform64(x, pm.A, pm.b)
    assert y.shape == (4000, 3) and (np.abs(y.astype(np.float64) - y64) <= _gamma(64) * mag).all()
    assert np.allclose(y.astype(np.float64).var(axis=0), ref.eigenvalues, rtol=1e-3)
    assert pm.apply_py(x[:9]).tobytes() == y[:9].tobytes()
    back = pm.reverse_transform(y)
    assert np.sqrt(((back - x).astype(np.float64) ** 2).mean()) <= 1.1 * np.sqrt(0.001)
    white = fi.PCAMatrix(64, 3, eigen_power=-0.5)
    white.train(x)
    assert np.allclose(white.apply(x).astype(np.float64).var(axis=0), 1.0, atol=2e-3)


# ----------------------------------------------------------------------------- HybridStorage.map on the HIP index
def test_map_on_the_hip_index(tmp_path):
    fi = _fi()
    from claude_semantic_search_amd.chunk import Chunk
    from claude_semantic_search_amd.storage import HybridStorage, MapPoint, StorageConfig
    from kmeans_fakes import planted

    d, sizes = 768, (150, 100, 50)
    lab = np.random.default_rng(3).permutation(np.repeat([0, 1, 2], sizes))
    n = lab.shape[0]
    C = planted(3, d, 3, seed=0)[2]
    x = (C[lab] + np.random.default_rng(4).integers(-2, 3, size=(n, d)) / 8.0).astype(np.float32)
    s = HybridStorage(StorageConfig(data_dir=str(tmp_path / "m"), embedding_dim=d, auto_save=False))
    s.initialize()
    s.add_chunks([Chunk(f"c{i}", f"text {i}", {"project_name": "alpha" if i % 3 else "beta", "session_id": f"s{lab[i]}"}, x[i])
                  for i in range(n)])

    def check(pts, allow):
        rows = np.flatnonzero(allow)
        assert [p.chunk_id for p in pts] == [f"c{i}" for i in rows] and all(isinstance(p, MapPoint) for p in pts)
        res = s.faiss_index.pca(2, allow=allow)
        b = fi.pca_offset(res.components, res.mean)
        y = s.faiss_index.transform(res.components, b)
        assert all((p.x, p.y) == (float(y[r, 0]), float(y[r, 1])) for p, r in zip(pts, rows))
        stored = s.faiss_index.reconstruct_n(0, n)               # (normalised on the device)
        y64, mag = transform64(stored, res.components, b)
        assert (np.abs(y.astype(np.float64) - y64) <= _gamma(d) * mag).all()
        ref = fi.pca_from_gram(*fi.fixed_point_gram(stored, allow, res.shift), res.shift, 2)
        assert res.components.tobytes() == ref.components.tobytes() and res.mean.tobytes() == ref.mean.tobytes()
        return np.array([(p.x, p.y) for p in pts])

    everything = np.ones(n, bool)
    xy = check(s.map(), everything)
    cen = np.stack([xy[lab == c].mean(axis=0) for c in range(3)])
    assert np.array_equal(((xy[:, None, :] - cen[None]) ** 2).sum(-1).argmin(axis=1), lab)   # the subjects are apart
    victim = int(np.flatnonzero(lab == 0)[0])
    assert s.delete_chunk(f"c{victim}")
    live = everything.copy()
    live[victim] = False
    check(s.map(), live)
    beta = live & (np.arange(n) % 3 == 0)
    check(s.map(filters={"project_name": "beta"}), beta)
    seed = next(sd for sd in range(64) if len(set(lab[fi.kmeans_init_ids(np.flatnonzero(live), 3, sd)].tolist())) == 3)
    pts = s.map(n_topics=3, seed=seed)
    topics = s.topics(n_topics=3, seed=seed)
    member = {c: k for k, t in enumerate(topics) for c in t.chunk_ids}
    pairs = {(p.topic, member[p.chunk_id]) for p in pts}
    assert len(pts) == n - 1 and len(pairs) == 3 == len({a for a, _ in pairs}) == len({b for _, b in pairs})
    assert {p.chunk_id: p.topic for p in pts if lab[int(p.chunk_id[1:])] == 2}.keys() == set(topics[2].chunk_ids)
    assert s.map(filters={"project_name": "nobody"}) == []
    s.close()


# ----------------------------------------------------------------------------- two ranks on one GPU
def _sharded_data():
    x = _unit(3001, 768, 55)
    x[2000:2300] *= np.float32(3.0)                              # longer rows on ONE shard: the global maximum sets the shift
    rng = np.random.default_rng(56)
    return x, rng.standard_normal((5, 768)).astype(np.float32), rng.standard_normal(5).astype(np.float32)


def _rank(rank, world, port, out_dir):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import torch
    import torch.distributed as dist

    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from claude_semantic_search_amd.sharded import ShardedFlatIndex

        torch.cuda.set_device(0)
        x, A, b = _sharded_data()
        sh = ShardedFlatIndex(768, 0, device_index=0)
        sh.add_global(x[:2000])
        sh.add_routed(x[2000:2300])
        sh.add_global(x[2300:])
        allow = np.arange(3001) % 3 != 0
        g = sh.gram(allow=allow)
        res = sh.pca(4, allow=allow)
        y = sh.transform(A, b, row0=900, n=1500)
        np.savez(os.path.join(out_dir, f"p{rank}.npz"), gram=g.gram, colsum=g.colsum, meta=np.array([g.count, g.shift]),
                 mean=res.mean, comp=res.components, eig=res.eigenvalues, y=y, mine=sh.local_rows_of(np.arange(3001)))
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
    x, A, b = _sharded_data()
    ix = fi.IndexFlatIP(768)
    ix.add(x)
    allow = np.arange(3001) % 3 != 0
    g = ix.gram(allow=allow)
    res = ix.pca(4, allow=allow)
    y = ix.transform(A, b, row0=900, n=1500)
    ix.close()
    sizes = []
    for r in range(2):
        got = np.load(tmp_path / f"p{r}.npz")
        assert np.array_equal(got["gram"], g.gram) and np.array_equal(got["colsum"], g.colsum), r
        assert got["meta"].tolist() == [g.count, g.shift], r
        assert got["mean"].tobytes() == res.mean.tobytes() and got["comp"].tobytes() == res.components.tobytes(), r
        assert np.array_equal(got["eig"], res.eigenvalues), r
        assert got["y"].tobytes() == y.tobytes(), r
        sizes.append(got["mine"].shape[0])
    assert sum(sizes) == 3001 and min(sizes) > 1000
