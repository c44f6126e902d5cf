"""CPU, world_size 2 over gloo: ``ShardedFlatIndex.search_prior`` / ``set_priors`` and the facade equal the unsharded
numpy double (``prior_fakes.FakePriorIndex``), ``(D, I, S)`` bit for bit.  Rows, priors and weights are multiples of
1/8, so every fused value is exact and ties are plentiful.  Covered: a ``set_priors`` range that straddles the shard
boundary, several segments per shard, an allow mask, tombstones, both metrics, a negative weight."""
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
KS = (1, 5, 16, 128)
WEIGHTS = (0.5, 2.0, -0.25)
N = 341


def _data():
    rng = np.random.default_rng(17)
    q = (rng.integers(-8, 9, size=(NQ, D_)) / 8.0).astype(np.float32)
    x = (rng.integers(-8, 9, size=(N, D_)) / 8.0).astype(np.float32)
    p = (rng.integers(0, 17, size=N) / 8.0).astype(np.float32)
    return q, x, p


def _cat(res):
    return np.concatenate([a.astype(np.float64) for a in res], axis=1)


def _worker(rank, world, port, out_dir):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from claude_semantic_search_amd.sharded import ShardedFlatIndex, ShardedIndexFacade
        from prior_fakes import FakePriorIndex
        from related_fakes import merge_lists

        q, x, p = _data()
        out = {}
        allow = (np.arange(N) % 4) != 1
        for metric in (0, 1):
            sh = ShardedFlatIndex(D_, metric, index_factory=lambda: FakePriorIndex(D_, metric), merge=merge_lists(metric))
            sh.add_global(x[:200])                        # rank 0: rows 0..99, rank 1: rows 100..199
            out[f"none{metric}"] = _cat(sh.search_prior(q, 16, 0.5))          # no prior set yet
            sh.set_priors(p[60:140], row0=60)             # a range that straddles the shard boundary
            out[f"part{metric}"] = _cat(sh.search_prior(q, 16, 0.5))
            sh.add_routed(x[200:241])
            sh.add_global(x[241:])
            assert len(sh.segments) >= 2
            sh.set_priors(p[:100])                        # the rest in two steps, the second with a row offset
            sh.set_priors(p[100:], row0=100)
            for k in KS:
                for w in WEIGHTS:
                    out[f"all{metric}_{k}_{w}"] = _cat(sh.search_prior(q, k, w))
                    out[f"mask{metric}_{k}_{w}"] = _cat(sh.search_prior(q, k, w, allow=allow))
            sh.mark_deleted([0, 7, 150, 220, 340])
            out[f"dead{metric}"] = _cat(sh.search_prior(q, 16, 0.5, allow=allow))
        fac = ShardedIndexFacade(D_, 0, index_factory=lambda: FakePriorIndex(D_, 0), merge=merge_lists(0))
        for lo in range(0, N, 31):
            fac.add(x[lo:lo + 31])
        fac.set_priors(p)
        fac.set_priors(p[300:], row0=300)
        out["fac"] = _cat(fac.search_prior(q, 16, 0.5))
        for bad in ((0, 0.5), (129, 0.5), (5, float("nan")), (5, float("inf"))):
            try:
                fac.search_prior(q, *bad)
                raise AssertionError(f"search_prior{bad} did not raise")
            except ValueError:
                pass
        try:
            fac.set_priors(p, row0=1)
            raise AssertionError("set_priors beyond the rows did not raise")
        except ValueError:
            pass
        np.savez(os.path.join(out_dir, f"p{rank}.npz"), **out)
    finally:
        dist.destroy_process_group()


def test_two_rank_prior_search_equals_the_unsharded_double(tmp_path):
    from prior_fakes import FakePriorIndex

    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    mp.spawn(_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    got = [np.load(tmp_path / f"p{r}.npz") for r in range(2)]
    q, x, p = _data()

    def whole(rows, priors, metric, k, w, allow=None):
        ix = FakePriorIndex(D_, metric)
        ix.add(rows)
        ix.set_priors(priors)
        return _cat(ix.search_prior(q, k, w, allow=allow))

    allow = (np.arange(N) % 4) != 1
    dead = allow.copy()
    dead[[0, 7, 150, 220, 340]] = False
    part = np.zeros(200, np.float32)
    part[60:140] = p[60:140]
    for r in range(2):
        for metric in (0, 1):
            assert np.array_equal(got[r][f"none{metric}"], whole(x[:200], np.zeros(200, np.float32), metric, 16, 0.5)), ("none", r, metric)
            assert np.array_equal(got[r][f"part{metric}"], whole(x[:200], part, metric, 16, 0.5)), ("part", r, metric)
            for k in KS:
                for w in WEIGHTS:
                    assert np.array_equal(got[r][f"all{metric}_{k}_{w}"], whole(x, p, metric, k, w)), ("all", r, metric, k, w)
                    assert np.array_equal(got[r][f"mask{metric}_{k}_{w}"], whole(x, p, metric, k, w, allow)), ("mask", r, metric, k, w)
            assert np.array_equal(got[r][f"dead{metric}"], whole(x, p, metric, 16, 0.5, dead)), ("dead", r, metric)
        assert np.array_equal(got[r]["fac"], whole(x, p, 0, 16, 0.5)), ("fac", r)
    # the cases are what they claim: the straddling range changed the answer, and rows of both shards are in it
    assert not np.array_equal(got[0]["part0"], got[0]["none0"])
    ids = got[0]["part0"][:, 16:32].astype(np.int64)
    assert (ids < 100).any() and (ids >= 100).any()
    # the fused order is not the plain one
    assert not np.array_equal(whole(x, p, 0, 16, 2.0)[:, 16:32], whole(x, np.zeros(N, np.float32), 0, 16, 2.0)[:, 16:32])
