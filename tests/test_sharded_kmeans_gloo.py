"""CPU, world_size 2 over gloo: ``ShardedFlatIndex.kmeans`` / ``reconstruct_batch`` and the facade equal ONE numpy double
(``kmeans_fakes.FakeKmeansIndex``) that holds all rows -- centroids, sizes and objective bit for bit, because every
shard sums in the fixed point of the GLOBAL shift and integers add up in any order.  Covered: several segments per
shard, one row far longer than the rest on one shard only (the global maximum decides the shift), an allow mask,
tombstones, a training subset, and the facade's assignment in global numbering."""
import os
import socket
import sys
from pathlib import Path

import numpy as np
import torch.distributed as dist
import torch.multiprocessing as mp

sys.path.insert(0, str(Path(__file__).resolve().parent))

D_ = 16
N = 413
NC = 5
DEAD = [3, 120, 250, 412]


def _data():
    from kmeans_fakes import planted

    x, lab, C = planted(N, D_, NC, seed=33)
    x[37] *= 16.0            # one long row (it lands on rank 0): the shift follows the GLOBAL maximum
    return x, lab, C


def _pack(res):
    return dict(c=res.centroids, sizes=res.sizes, obj=np.array(res.obj, np.float64), it=np.array([res.iterations]),
                a=res.assign, d=res.dist)


def _worker(rank, world, port, out_dir):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from claude_semantic_search_amd.sharded import ShardedFlatIndex, ShardedIndexFacade
        from kmeans_fakes import FakeKmeansIndex
        from related_fakes import merge_lists

        x, lab, C = _data()
        out = {}
        sh = ShardedFlatIndex(D_, 1, index_factory=lambda: FakeKmeansIndex(D_, 1), merge=merge_lists(1))
        sh.add_global(x[:200])
        sh.add_routed(x[200:241])
        sh.add_global(x[241:])
        assert len(sh.segments) >= 2
        ids = np.array([0, 412, 150, 150, 220, 99, 100], np.int64)
        out["rows"] = sh.reconstruct_batch(ids)
        for key, kw in (("plain", {}), ("seeded", dict(seed=7, init=None)), ("sph", dict(spherical=True)),
                        ("mask", dict(allow=(np.arange(N) % 4) != 1)), ("sub", dict(max_points_per_centroid=20, seed=3))):
            kw = dict(dict(init=C + np.float32(0.25), niter=6), **kw)
            res = sh.kmeans(NC, **kw)
            for name, v in _pack(res).items():
                out[f"{key}_{name}"] = v
            out[f"{key}_local"] = sh.local_rows_of(np.arange(N))        # which global rows the local values belong to
        sh.mark_deleted(DEAD)
        for name, v in _pack(sh.kmeans(NC, init=C, niter=4)).items():
            out[f"dead_{name}"] = v
        out["dead_local"] = sh.local_rows_of(np.arange(N))
        fac = ShardedIndexFacade(D_, 1, index_factory=lambda: FakeKmeansIndex(D_, 1), merge=merge_lists(1))
        for lo in range(0, N, 31):
            fac.add(x[lo:lo + 31])
        for name, v in _pack(fac.kmeans(NC, init=C, niter=4)).items():
            out[f"fac_{name}"] = v
        out["fac_rows"] = fac.reconstruct_batch(ids)
        try:
            sh.reconstruct_batch([N])
            raise AssertionError("an id beyond the rows did not raise")
        except ValueError:
            pass
        try:
            sh.kmeans(NC, allow=np.arange(N) < 3)
            raise AssertionError("fewer allowed rows than centroids did not raise")
        except ValueError:
            pass
        np.savez(os.path.join(out_dir, f"k{rank}.npz"), **out)
    finally:
        dist.destroy_process_group()


def test_two_rank_kmeans_equals_one_double_bit_for_bit(tmp_path):
    from kmeans_fakes import FakeKmeansIndex

    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    mp.spawn(_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    got = [np.load(tmp_path / f"k{r}.npz") for r in range(2)]
    x, lab, C = _data()
    whole = FakeKmeansIndex(D_, 1)
    whole.add(x)
    ids = np.array([0, 412, 150, 150, 220, 99, 100], np.int64)
    dead = np.ones(N, bool)
    dead[DEAD] = False
    cases = {"plain": {}, "seeded": dict(seed=7, init=None), "sph": dict(spherical=True),
             "mask": dict(allow=(np.arange(N) % 4) != 1), "sub": dict(max_points_per_centroid=20, seed=3)}
    for r in range(2):
        assert np.array_equal(got[r]["rows"], x[ids]) and np.array_equal(got[r]["fac_rows"], x[ids])
        for key, kw in cases.items():
            ref = whole.kmeans(NC, **dict(dict(init=C + np.float32(0.25), niter=6), **kw))
            assert np.array_equal(got[r][f"{key}_c"], ref.centroids), (key, r)
            assert np.array_equal(got[r][f"{key}_sizes"], ref.sizes), (key, r)
            assert np.array_equal(got[r][f"{key}_obj"], np.array(ref.obj, np.float64)), (key, r)
            assert int(got[r][f"{key}_it"][0]) == ref.iterations
            mine = got[r][f"{key}_local"]
            assert np.array_equal(got[r][f"{key}_a"], ref.assign[mine]) and np.array_equal(got[r][f"{key}_d"], ref.dist[mine])
        ref = whole.kmeans(NC, init=C, niter=4, allow=dead)
        assert np.array_equal(got[r]["dead_c"], ref.centroids) and np.array_equal(got[r]["dead_sizes"], ref.sizes)
        assert np.array_equal(got[r]["dead_a"], ref.assign[got[r]["dead_local"]])
        assert int(ref.sizes.sum()) == N - len(DEAD)
        ref = whole.kmeans(NC, init=C, niter=4)
        assert np.array_equal(got[r]["fac_c"], ref.centroids) and np.array_equal(got[r]["fac_sizes"], ref.sizes)
        assert np.array_equal(got[r]["fac_a"], ref.assign) and np.array_equal(got[r]["fac_d"], ref.dist)   # global numbering
    # the cases are what they claim: both shards hold rows of the local lists, and the long row moved the shift
    assert 0 < got[0]["plain_a"].shape[0] < N and got[0]["plain_a"].shape[0] + got[1]["plain_a"].shape[0] == N
    from claude_semantic_search_amd import flat_index as fi
    short = x.copy()
    short[37] /= 16.0
    n2 = lambda a: float((a.astype(np.float64) ** 2).sum(axis=1).max())   # noqa: E731
    assert fi.kmeans_shift(n2(x), N)[0] < fi.kmeans_shift(n2(short), N)[0]
    assert not np.array_equal(got[0]["mask_sizes"], got[0]["plain_sizes"])
