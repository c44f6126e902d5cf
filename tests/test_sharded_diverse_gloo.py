"""CPU, world_size 2 over gloo: ``ShardedFlatIndex.search_diverse`` and the facade equal the unsharded numpy double
(``diverse_fakes.FakeDiverseIndex``, whose selection is the loop statement ``mmr_loop``) bit for bit, on both ranks.  Rows
are multiples of 1/8 and weights multiples of 1/4, so every score and similarity is exact and ties are plentiful; a third
of the rows are copies of other rows, so the selection has something to push apart.  One case keeps the rows in one add
(the pool's rows then sit on both shards: checked), one goes through several segments per shard, masks and tombstones."""
import os
import socket
import sys
from pathlib import Path

import numpy as np
import torch.distributed as dist
import torch.multiprocessing as mp

sys.path.insert(0, str(Path(__file__).resolve().parent))

D_ = 8
NQ = 4
CASES = ((1, 0, 0.5), (5, 0, 0.5), (10, 0, 0.25), (10, 32, 0.75), (32, 32, 0.5), (20, 128, 0.0), (7, 128, 1.0))   # k, fetch, lam


def _data():
    rng = np.random.default_rng(11)
    q = (rng.integers(-8, 9, size=(NQ, D_)) / 8.0).astype(np.float32)
    xa = (rng.integers(-8, 9, size=(300, D_)) / 8.0).astype(np.float32)
    xa[200:] = xa[rng.permutation(200)[:100]]                 # copies, most of them on the other shard
    xb = (rng.integers(-8, 9, size=(341, D_)) / 8.0).astype(np.float32)
    xb[230:] = xb[rng.permutation(230)[:111]]
    return q, xa, xb


def _cat(res):
    return np.concatenate([a.astype(np.float64) for a in res], axis=1)


def _worker(rank, world, port, out_dir):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from claude_semantic_search_amd.sharded import ShardedFlatIndex, ShardedIndexFacade
        from diverse_fakes import FakeDiverseIndex
        from related_fakes import merge_lists

        q, xa, xb = _data()
        out = {}
        for metric in (0, 1):
            sh = ShardedFlatIndex(D_, metric, index_factory=lambda: FakeDiverseIndex(D_, metric), merge=merge_lists(metric))
            sh.add_global(xa)
            for k, fetch, lam in CASES:
                out[f"a{metric}_{k}_{fetch}"] = _cat(sh.search_diverse(q, k, lam=lam, fetch=fetch))
            sh = ShardedFlatIndex(D_, metric, index_factory=lambda: FakeDiverseIndex(D_, metric), merge=merge_lists(metric))
            sh.add_global(xb[:200])
            sh.add_routed(xb[200:241])
            sh.add_global(xb[241:])
            assert len(sh.segments) >= 2
            allow = (np.arange(341) % 4) != 1
            for k, fetch, lam in CASES:
                out[f"b{metric}_{k}_{fetch}"] = _cat(sh.search_diverse(q, k, lam=lam, fetch=fetch))
                out[f"bm{metric}_{k}_{fetch}"] = _cat(sh.search_diverse(q, k, lam=lam, fetch=fetch, allow=allow))
            few = np.zeros(341, bool)
            few[[3, 100, 101, 250, 340]] = True                # a pool shorter than k: pads behind five picks
            out[f"bf{metric}"] = _cat(sh.search_diverse(q, 10, allow=few))
            sh.mark_deleted([0, 7, 150, 220, 340])
            out[f"bd{metric}"] = _cat(sh.search_diverse(q, 10, lam=0.5, fetch=128, allow=allow))
            out[f"e{metric}"] = _cat(sh.search_diverse(q[:0], 3))
        fac = ShardedIndexFacade(D_, 0, index_factory=lambda: FakeDiverseIndex(D_, 0), merge=merge_lists(0))
        for lo in range(0, 341, 31):
            fac.add(xb[lo:lo + 31])
        out["fac"] = _cat(fac.search_diverse(q, 10, lam=0.5, fetch=128))
        np.savez(os.path.join(out_dir, f"d{rank}.npz"), **out)
    finally:
        dist.destroy_process_group()


def test_two_rank_diversified_search_equals_the_unsharded_double(tmp_path):
    from diverse_fakes import FakeDiverseIndex

    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    mp.spawn(_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    got = [np.load(tmp_path / f"d{r}.npz") for r in range(2)]
    q, xa, xb = _data()

    def whole(x, metric, k, fetch=0, lam=0.5, allow=None):
        ix = FakeDiverseIndex(D_, metric)
        ix.add(x)
        return _cat(ix.search_diverse(q, k, lam=lam, fetch=fetch, allow=allow))

    allow = (np.arange(341) % 4) != 1
    dead = allow.copy()
    dead[[0, 7, 150, 220, 340]] = False
    few = np.zeros(341, bool)
    few[[3, 100, 101, 250, 340]] = True
    for r in range(2):
        for metric in (0, 1):
            for k, fetch, lam in CASES:
                key = f"{metric}_{k}_{fetch}"
                assert np.array_equal(got[r]["a" + key], whole(xa, metric, k, fetch, lam)), ("a", r, key)
                assert np.array_equal(got[r]["b" + key], whole(xb, metric, k, fetch, lam)), ("b", r, key)
                assert np.array_equal(got[r]["bm" + key], whole(xb, metric, k, fetch, lam, allow)), ("bm", r, key)
            assert np.array_equal(got[r][f"bf{metric}"], whole(xb, metric, 10, allow=few)), ("bf", r, metric)
            assert (got[r][f"bf{metric}"][:, 15:] == -1).all() and (got[r][f"bf{metric}"][:, 10:15] >= 0).all()
            assert np.array_equal(got[r][f"bd{metric}"], whole(xb, metric, 10, 128, 0.5, dead)), ("bd", r, metric)
            assert got[r][f"e{metric}"].shape == (0, 6)
        assert np.array_equal(got[r]["fac"], whole(xb, 0, 10, 128, 0.5)), ("fac", r)
    # case (a) is what it claims: the picks of every query come from both shards (rows 0..149 | 150..299), and the
    # selection did something -- the picks are not the head of the ranking
    picks = whole(xa, 0, 10, 0, 0.25)[:, 10:].astype(np.int64)
    assert all((row < 150).any() and (row >= 150).any() for row in picks)
    assert not np.array_equal(picks, whole(xa, 0, 10, 0, 1.0)[:, 10:].astype(np.int64))
