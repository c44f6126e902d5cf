"""CPU, world_size 2 over gloo: ``ShardedFlatIndex.search_by_ids`` / ``ShardedIndexFacade.search_by_ids`` (the owner's
row through one sum all-reduce -> the usual search for ``k + 1`` -> the anchor dropped after the merge) equals ONE
unsharded index, for both metrics, with several segments per shard, anchors owned by either rank, an anchor whose
copies live on the other rank, allow masks and tombstones.  The local indexes are the numpy double of
``related_fakes`` (its ``search_by_ids`` is stated without the ``k + 1`` detour, so the comparison means something);
rows are multiples of 1/8, every score is exact in float32, and ties are plentiful."""
import os
import socket

import numpy as np
import pytest
import torch.distributed as dist
import torch.multiprocessing as mp

from related_fakes import FakeIndex, merge_lists

D_ = 16
ADDS = ((40, "global"), (7, "routed"), (3, "routed"), (50, "global"))      # 100 rows, several segments per shard
# rank 0 owns rows 0..19, 40..46 and 50..74; rank 1 owns 20..39, 47..49 and 75..99
ANCHORS = np.array([3, 30, 44, 48, 60, 99, 3], np.int64)                   # either rank, every add, one repeated
K = 6


def _data():
    x = (np.random.default_rng(5).integers(-4, 5, size=(100, D_)) / 8).astype(np.float32)
    x[25] = x[3]          # copies of anchor 3 (rank 0) live on rank 1 ...
    x[80] = x[3]
    x[10] = x[99]         # ... and a copy of anchor 99 (rank 1) on rank 0
    return x


def _build(cls_or_sharded, x):
    r0 = 0
    for n, how in ADDS:
        (cls_or_sharded.add_global if how == "global" else cls_or_sharded.add_routed)(x[r0:r0 + n])
        r0 += n


def _worker(rank, world, port, out_dir):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from claude_semantic_search_amd.sharded import ShardedFlatIndex, ShardedIndexFacade

        x = _data()
        out = {}
        for metric in (0, 1):
            sh = ShardedFlatIndex(D_, metric, index_factory=lambda: FakeIndex(D_, metric), merge=merge_lists(metric))
            _build(sh, x)
            assert sh.ntotal_global == 100 and len(sh.segments) >= 2 and sh.local.ntotal == sh.shard_sizes[rank]
            owned = np.zeros(100, bool)
            for l0, g0, n in sh.segments:
                owned[g0:g0 + n] = True
            assert owned[3] == (rank == 0) and owned[25] == (rank == 1) and owned[99] == (rank == 1) and owned[10] == (rank == 0)
            out[f"m{metric}"] = sh.search_by_ids(ANCHORS, K)
            out[f"m{metric}self"] = sh.search_by_ids(ANCHORS, K, exclude_self=False)
            out[f"m{metric}big"] = sh.search_by_ids(ANCHORS[:2], 99)
            allow = (np.arange(100) % 3) != 0                                   # anchors 3, 30, 48, 60 and 99 masked out
            out[f"m{metric}allow"] = sh.search_by_ids(ANCHORS, K, allow=allow)
            sh.mark_deleted([25, 61])
            out[f"m{metric}dead"] = sh.search_by_ids(ANCHORS, K, allow=allow)
            out[f"m{metric}none"] = sh.search_by_ids([], K)
            for bad in ([100], [-1], [5, 1000]):                                # raises on every rank, before any collective
                with pytest.raises(ValueError):
                    sh.search_by_ids(bad, K)
            with pytest.raises(ValueError):
                sh.search_by_ids([0.5], K)
        fac = ShardedIndexFacade(D_, 0, index_factory=lambda: FakeIndex(D_, 0), merge=merge_lists(0))
        fac.add(x[:10])
        fac.add(x[10:30])
        out["facade"] = fac.search_by_ids([3, 25, 12], 4)
        np.savez(os.path.join(out_dir, f"r{rank}.npz"), **{f"{k}_{n}": v for k, t in out.items() for n, v in zip("DI", t)})
    finally:
        dist.destroy_process_group()


def _one(x, metric):
    ix = FakeIndex(D_, metric)
    ix.add(x)
    return ix


def test_two_rank_search_by_ids_equals_one_index(tmp_path):
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    mp.spawn(_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    x = _data()
    got = [np.load(tmp_path / f"r{r}.npz") for r in range(2)]

    def same(key, want, what):
        for r in range(2):
            for n, w in zip("DI", want):
                g = got[r][f"{key}_{n}"]
                assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), f"rank {r} {what}: {n} differs"

    for metric in (0, 1):
        one = _one(x, metric)
        want = one.search_by_ids(ANCHORS, K)
        same(f"m{metric}", want, f"metric {metric}")
        # the copies on the other rank come back with the self score, the anchor never does
        assert set(want[1][0, :2].tolist()) == {25, 80} and want[1][5, 0] == 10
        assert not (want[1] == ANCHORS[:, None]).any()
        same(f"m{metric}self", one.search(x[ANCHORS], K), f"metric {metric}, exclude_self=False")
        same(f"m{metric}big", one.search_by_ids(ANCHORS[:2], 99), f"metric {metric}, every other row")
        allow = (np.arange(100) % 3) != 0
        same(f"m{metric}allow", one.search_by_ids(ANCHORS, K, allow=allow), "allow mask")
        dead = allow.copy()
        dead[[25, 61]] = False
        same(f"m{metric}dead", one.search_by_ids(ANCHORS, K, allow=dead), "allow mask and tombstones")
        same(f"m{metric}none", (np.empty((0, K), np.float32), np.empty((0, K), np.int64)), "no anchors")
    same("facade", _one(x[:30], 0).search_by_ids([3, 25, 12], 4), "facade")


def test_single_process_skips_the_collectives():
    """World 1 (no process group): the row comes from the local index, ids go through the segment table."""
    from claude_semantic_search_amd.sharded import ShardedFlatIndex

    x = _data()
    sh = ShardedFlatIndex(D_, 0, index_factory=lambda: FakeIndex(D_, 0), merge=merge_lists(0))
    sh.add_global(x[:60])
    sh.add_routed(x[60:])
    D, I = sh.search_by_ids(ANCHORS, K)
    want = _one(x, 0).search_by_ids(ANCHORS, K)
    assert np.array_equal(D, want[0]) and np.array_equal(I, want[1])
    with pytest.raises(ValueError):
        sh.search_by_ids([100], K)
    with pytest.raises(ValueError):
        sh.search_by_ids([1], 2048)
