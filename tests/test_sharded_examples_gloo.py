"""CPU, world_size 2 over gloo: ``ShardedFlatIndex.search_examples`` and the facade equal the unsharded numpy double
(``examples_fakes.FakeExamplesIndex``), ``(D, I, S)`` bit for bit.  Rows, examples and gammas are multiples of 1/8, so
every fused value is exact and ties are plentiful.  Covered: id examples owned by either rank (and by both at once),
vector examples, exclusion on and off, several segments per shard, an allow mask, tombstones, both metrics."""
import os
import socket
import sys
from pathlib import Path

import numpy as np
import torch.distributed as dist
import torch.multiprocessing as mp

sys.path.insert(0, str(Path(__file__).resolve().parent))

D_ = 8
KS = (1, 5, 16, 100)
GAMMAS = (0.0, 0.5, 2.0)
N = 341
# (positive vectors, negative vectors, positive ids, negative ids): rows 0..99 and 200.. start on rank 0, 100..199 on rank 1
REQUESTS = (((0,), (), (), ()), ((), (), (7,), ()), ((), (), (150,), ()), ((), (), (7, 150), (260,)), ((0, 1), (2,), (120,), (30, 330)),
            ((3,), (4, 5), (), (199,)), ((), (), (0, 100, 340), (99, 101)), ((1,), (), (7, 7), (150,)))


def _data():
    rng = np.random.default_rng(23)
    v = (rng.integers(-8, 9, size=(6, D_)) / 8.0).astype(np.float32)
    x = (rng.integers(-8, 9, size=(N, D_)) / 8.0).astype(np.float32)
    return v, x


def _cat(res):
    return np.concatenate([a.astype(np.float64) for a in res])


def _call(ix, v, req, k, gamma, **kw):
    vp, vn, ip, ineg = req
    return _cat(ix.search_examples(v[list(vp)], v[list(vn)], list(ip), list(ineg), k=k, gamma=gamma, **kw))


def _worker(rank, world, port, out_dir):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from claude_semantic_search_amd.sharded import ShardedFlatIndex, ShardedIndexFacade
        from examples_fakes import FakeExamplesIndex
        from related_fakes import merge_lists

        v, x = _data()
        out = {}
        allow = (np.arange(N) % 4) != 1
        for metric in (0, 1):
            sh = ShardedFlatIndex(D_, metric, index_factory=lambda: FakeExamplesIndex(D_, metric), merge=merge_lists(metric))
            sh.add_global(x[:200])                        # rank 0: rows 0..99, rank 1: rows 100..199
            sh.add_routed(x[200:241])
            sh.add_global(x[241:])
            assert len(sh.segments) >= 2
            for t, req in enumerate(REQUESTS):
                for k in KS:
                    for g in GAMMAS:
                        out[f"all{metric}_{t}_{k}_{g}"] = _call(sh, v, req, k, g)
                out[f"keep{metric}_{t}"] = _call(sh, v, req, 16, 0.5, exclude_ids=False)
                out[f"mask{metric}_{t}"] = _call(sh, v, req, 16, 0.5, allow=allow)
            sh.mark_deleted([0, 7, 150, 220, 340])        # (tombstoned rows still serve as examples)
            for t, req in enumerate(REQUESTS):
                out[f"dead{metric}_{t}"] = _call(sh, v, req, 16, 0.5, allow=allow)
            # local calls: every example as a vector, nothing excluded on the device, k + ids rows
            last = sh.local.calls[-1]
            assert last[0] == "search_examples" and last[1] == 16 + 3 and last[3:] == (3, 1, False), last
        fac = ShardedIndexFacade(D_, 0, index_factory=lambda: FakeExamplesIndex(D_, 0), merge=merge_lists(0))
        for lo in range(0, N, 31):
            fac.add(x[lo:lo + 31])
        out["fac"] = _call(fac, v, REQUESTS[4], 16, 0.5)
        for bad in (dict(k=0), dict(k=129), dict(gamma=float("nan")), dict(gamma=-1.0), dict(pos_ids=[N]), dict(neg_ids=[-1]),
                    dict(k=120, pos_ids=list(range(9)))):          # k + ids beyond 128
            try:
                fac.search_examples(**{"pos": v[:1], "k": 5, **bad})
                raise AssertionError(f"search_examples({bad}) did not raise")
            except ValueError:
                pass
        try:
            fac.search_examples(neg=v[:1], k=5)
            raise AssertionError("no positive did not raise")
        except ValueError:
            pass
        np.savez(os.path.join(out_dir, f"e{rank}.npz"), **out)
    finally:
        dist.destroy_process_group()


def test_two_rank_example_search_equals_the_unsharded_double(tmp_path):
    from examples_fakes import FakeExamplesIndex

    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    mp.spawn(_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    got = [np.load(tmp_path / f"e{r}.npz") for r in range(2)]
    v, x = _data()
    allow = (np.arange(N) % 4) != 1
    dead = allow.copy()
    dead[[0, 7, 150, 220, 340]] = False
    for metric in (0, 1):
        ix = FakeExamplesIndex(D_, metric)
        ix.add(x)
        for r in range(2):
            for t, req in enumerate(REQUESTS):
                for k in KS:
                    for g in GAMMAS:
                        assert np.array_equal(got[r][f"all{metric}_{t}_{k}_{g}"], _call(ix, v, req, k, g)), ("all", r, metric, t, k, g)
                assert np.array_equal(got[r][f"keep{metric}_{t}"], _call(ix, v, req, 16, 0.5, exclude_ids=False)), ("keep", r, metric, t)
                assert np.array_equal(got[r][f"mask{metric}_{t}"], _call(ix, v, req, 16, 0.5, allow=allow)), ("mask", r, metric, t)
                assert np.array_equal(got[r][f"dead{metric}_{t}"], _call(ix, v, req, 16, 0.5, allow=dead)), ("dead", r, metric, t)
        if metric == 0:
            for r in range(2):
                assert np.array_equal(got[r]["fac"], _call(ix, v, REQUESTS[4], 16, 0.5)), ("fac", r)
    # the cases are what they claim: rows of both shards are in an answer, the example ids are not, and without the
    # exclusion the positive anchor is in it
    ids = got[0]["all0_3_16_0.5"][16:32].astype(np.int64)
    assert (ids < 100).any() and ((ids >= 100) & (ids < 200)).any() and not np.isin(ids, [7, 150, 260]).any()
    assert 7 in got[0]["keep1_1"][16:32].astype(np.int64) and got[0]["keep1_1"][0] == 0.0     # (L2: distance 0)
    assert 7 not in got[0]["all1_1_16_0.5"][16:32].astype(np.int64)
    # the negatives reorder
    assert not np.array_equal(got[0]["all0_3_16_2.0"][16:32], got[0]["all0_3_16_0.0"][16:32])
