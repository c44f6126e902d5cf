"""CPU, world_size 2 over gloo: ``ShardedFlatIndex.search_grouped`` / ``set_groups`` and the facade equal the
unsharded numpy double (``grouped_fakes.FakeGroupedIndex``) bit for bit.  Rows are multiples of 1/8, so scores are exact
and ties are plentiful.  One case puts the best rows of all the top groups on ONE shard, one lets groups straddle both
shards (best row on one, other rows on the other), and both go through several segments per shard, masks and tombstones."""
import os
import socket
import sys
from pathlib import Path

import numpy as np
import torch.distributed as dist
import torch.multiprocessing as mp

sys.path.insert(0, str(Path(__file__).resolve().parent))

D_ = 8
NQ = 6
KS = (1, 5, 16, 40)


def _data():
    rng = np.random.default_rng(7)
    q = (rng.integers(-8, 9, size=(NQ, D_)) / 8.0).astype(np.float32)
    # (a) rows 0..149 score high against every query's direction mix, rows 150.. are small: with add_global in ONE call
    #     rank 0 keeps the first half, so the best rows of the top groups all lie on shard 0
    xa = (rng.integers(-8, 9, size=(300, D_)) / 8.0).astype(np.float32)
    xa[150:] *= 0.125
    ga = rng.integers(0, 30, size=300).astype(np.int32)
    ga[rng.random(300) < 0.1] = -1
    # (b) three adds (several segments per shard); labels drawn over ALL rows, so groups straddle the shards
    xb = (rng.integers(-8, 9, size=(341, D_)) / 8.0).astype(np.float32)
    gb = rng.integers(0, 25, size=341).astype(np.int32)
    gb[rng.random(341) < 0.15] = -5           # any negative label: ungrouped
    return q, xa, ga, xb, gb


def _worker(rank, world, port, out_dir):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from claude_semantic_search_amd.sharded import ShardedFlatIndex, ShardedIndexFacade
        from grouped_fakes import FakeGroupedIndex
        from related_fakes import merge_lists

        q, xa, ga, xb, gb = _data()
        out = {}
        for metric in (0, 1):
            sh = ShardedFlatIndex(D_, metric, index_factory=lambda: FakeGroupedIndex(D_, metric), merge=merge_lists(metric))
            sh.add_global(xa)
            sh.set_groups(ga)
            for k in KS:
                out[f"a{metric}_{k}"] = np.concatenate([a.astype(np.float64) for a in sh.search_grouped(q, k)], axis=1)
            sh = ShardedFlatIndex(D_, metric, index_factory=lambda: FakeGroupedIndex(D_, metric), merge=merge_lists(metric))
            sh.add_global(xb[:200])
            sh.add_routed(xb[200:241])
            sh.add_global(xb[241:])
            assert len(sh.segments) >= 2
            sh.set_groups(gb[:100])                      # in two steps, the second with a row offset
            sh.set_groups(gb[100:], row0=100)
            allow = (np.arange(341) % 4) != 1
            for k in KS:
                out[f"b{metric}_{k}"] = np.concatenate([a.astype(np.float64) for a in sh.search_grouped(q, k)], axis=1)
                out[f"bm{metric}_{k}"] = np.concatenate([a.astype(np.float64) for a in sh.search_grouped(q, k, allow=allow)], axis=1)
            sh.mark_deleted([0, 7, 150, 220, 340])
            out[f"bd{metric}"] = np.concatenate([a.astype(np.float64) for a in sh.search_grouped(q, 16, allow=allow)], axis=1)
        # the facade: adds are routed whole, labels are set in global numbering
        fac = ShardedIndexFacade(D_, 0, index_factory=lambda: FakeGroupedIndex(D_, 0), merge=merge_lists(0))
        for lo in range(0, 341, 31):
            fac.add(xb[lo:lo + 31])
        fac.set_groups(gb)
        fac.set_groups(gb[300:], row0=300)
        out["fac"] = np.concatenate([a.astype(np.float64) for a in fac.search_grouped(q, 16)], axis=1)
        np.savez(os.path.join(out_dir, f"g{rank}.npz"), **out)
    finally:
        dist.destroy_process_group()


def test_two_rank_grouped_search_equals_the_unsharded_double(tmp_path):
    from grouped_fakes import FakeGroupedIndex

    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    mp.spawn(_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    got = [np.load(tmp_path / f"g{r}.npz") for r in range(2)]
    q, xa, ga, xb, gb = _data()

    def whole(x, g, metric, k, allow=None):
        ix = FakeGroupedIndex(D_, metric)
        ix.add(x)
        ix.set_groups(g)
        return np.concatenate([a.astype(np.float64) for a in ix.search_grouped(q, k, allow=allow)], axis=1)

    allow = (np.arange(341) % 4) != 1
    dead = allow.copy()
    dead[[0, 7, 150, 220, 340]] = False
    for r in range(2):
        for metric in (0, 1):
            for k in KS:
                assert np.array_equal(got[r][f"a{metric}_{k}"], whole(xa, ga, metric, k)), ("a", r, metric, k)
                assert np.array_equal(got[r][f"b{metric}_{k}"], whole(xb, gb, metric, k)), ("b", r, metric, k)
                assert np.array_equal(got[r][f"bm{metric}_{k}"], whole(xb, gb, metric, k, allow)), ("bm", r, metric, k)
            assert np.array_equal(got[r][f"bd{metric}"], whole(xb, gb, metric, 16, dead)), ("bd", r, metric)
        assert np.array_equal(got[r]["fac"], whole(xb, gb, 0, 16)), ("fac", r)
    # case (a) is what it claims: for the inner product the best rows of the top five groups all lie on shard 0
    ids = whole(xa, ga, 0, 5)[:, 5:10]
    assert (ids < 150).all()
    # case (b): some group of the answer has rows on both shards of the first add (rows 0..99 | 100..199)
    top = whole(xb, gb, 0, 16)[:, 32:].astype(np.int64)
    assert any(((gb[:100] == g).any() and (gb[100:200] == g).any()) for g in top[0] if g >= 0)
