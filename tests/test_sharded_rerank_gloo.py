"""CPU, world_size 2 over gloo: ``ShardedFlatIndex.maxsim_ids_batch`` / ``search_rerank_maxsim`` and the facade equal
the unsharded numpy double (``rerank_fakes.FakeRerankIndex``), bit for bit, with and without masks.  The data are those
of tests/test_sharded_tokens_gloo.py: lattice components (dense rows and tokens), twins on both sides of the shard
boundary, so that late scores tie inside a pool across the boundary and the position rule decides."""
import os
import socket
import sys
from pathlib import Path

import numpy as np
import torch.distributed as dist
import torch.multiprocessing as mp

sys.path.insert(0, str(Path(__file__).resolve().parent))

import test_sharded_tokens_gloo as base   # noqa: E402

D_, N, P = base.D_, base.N, base.P
ORDER = (2, 0, 3, 1, 2, 2, 0)   # 7 queries: equal ones in different places
SHAPES = ((1, 1), (10, 50), (50, 50), (128, 341), (16, 400))   # (k, fetch): below, at and above the 341 rows


def _queries():
    return (np.random.default_rng(32).integers(-8, 9, size=(len(ORDER), D_)) / 8.0).astype(np.float32)


def _floor():
    """The 26th best inner product of query 0: a floor equal to a pool score, in the middle of a pool of 50."""
    return float(np.sort(_queries()[0].astype(np.float64) @ base._data()[0].astype(np.float64).T)[::-1][25])


def _cat(res):
    return np.concatenate([np.ascontiguousarray(a).view(np.uint8).reshape(a.shape[0], -1).astype(np.float64) for a in res], axis=1)


def _searches(ix, qs, out, tag, allow=None):
    Q, mats = _queries(), [qs[i] for i in ORDER]
    for k, fetch in SHAPES:
        for floor in (None, _floor()):
            out[f"{tag}_{k}_{fetch}_{floor}"] = _cat(ix.search_rerank_maxsim(Q, mats, k, fetch, floor=floor, allow=allow))
    ids = np.array([[340, 0, 100, 99, 7, 100, 250, 199, -1, N + 3]] * len(ORDER), np.int64)
    ids[1::2] = ids[1::2, ::-1]
    ntotal = getattr(ix, "ntotal_global", None) or ix.ntotal
    ids[(ids >= ntotal)] = -1
    out[f"{tag}_lists"] = _cat((ix.maxsim_ids_batch(mats, ids),))


def _worker(rank, world, port, out_dir):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from claude_semantic_search_amd.sharded import ShardedFlatIndex, ShardedIndexFacade
        from related_fakes import merge_lists
        from rerank_fakes import FakeRerankIndex

        x, mats, qs = base._data()
        out = {}
        allow = (np.arange(N) % 4) != 1
        for metric in (0, 1):
            sh = ShardedFlatIndex(D_, metric, index_factory=lambda: FakeRerankIndex(D_, metric), merge=merge_lists(metric))
            sh.add_global(x[:200])
            sh.set_tokens(mats[:60])                                           # rank 1 is a shard without matrices
            sh.set_tokens(mats[60:200])
            sh.add_routed(x[200:241])
            sh.add_global(x[241:])
            sh.set_tokens(mats[200:])
            _searches(sh, qs, out, f"all{metric}")
            _searches(sh, qs, out, f"mask{metric}", allow=allow)
            calls = [c[0] for c in sh.local.calls]
            assert "maxsim_ids_batch" in calls and "maxsim_ids" not in calls   # one list call per rank, no single calls
        fac = ShardedIndexFacade(D_, 0, index_factory=lambda: FakeRerankIndex(D_, 0), merge=merge_lists(0))
        for lo in range(0, N, 31):
            fac.add(x[lo:lo + 31])
        fac.set_tokens(mats)
        _searches(fac, qs, out, "fac", allow=allow)
        Q, batch = _queries(), [qs[i] for i in ORDER]
        for call in (lambda: fac.search_rerank_maxsim(Q, batch, 51, 50), lambda: fac.search_rerank_maxsim(Q[:3], batch, 5, 50),
                     lambda: fac.search_rerank_maxsim(Q, batch, 5, 2049), lambda: fac.maxsim_ids_batch(batch, [[1, 2]])):
            try:
                call()
                raise AssertionError("a bad call did not raise")
            except ValueError:
                pass
        np.savez(os.path.join(out_dir, f"p{rank}.npz"), **out)
    finally:
        dist.destroy_process_group()


def test_two_rank_two_stage_search_equals_the_unsharded_double(tmp_path):
    from rerank_fakes import FakeRerankIndex

    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    mp.spawn(_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    got = [np.load(tmp_path / f"p{r}.npz") for r in range(2)]
    x, mats, qs = base._data()
    allow = (np.arange(N) % 4) != 1
    for metric in (0, 1):
        ix = FakeRerankIndex(D_, metric)
        ix.add(x)
        ix.set_tokens(mats)
        want = {}
        _searches(ix, qs, want, f"all{metric}")
        _searches(ix, qs, want, f"mask{metric}", allow=allow)
        if metric == 0:
            _searches(ix, qs, want, "fac", allow=allow)
        for r in range(2):
            for key, val in want.items():
                assert got[r][key].shape == val.shape and np.array_equal(got[r][key], val), (key, r)
    # the cases are what they claim: rows of both shards, late ties inside a pool, padding above ntotal, the mask bites
    D_I = got[0]["all0_128_341_None"]
    ids = np.ascontiguousarray(D_I[:, 4 * 128:12 * 128].astype(np.uint8)).view(np.int64)
    late = np.ascontiguousarray(D_I[:, :4 * 128].astype(np.uint8)).view(np.float32)
    assert (ids[ids >= 0] < 100).any() and (ids >= 100).any()
    twins = [list(row[:len(base.TWINS)]) for row in ids]
    assert sorted(twins[0]) == sorted(base.TWINS) and (late[0, :len(base.TWINS)] == late[0, 0]).all()   # query 2: the twins tie
    assert twins[0] != sorted(twins[0])                                                                # ... in POOL order
    assert not np.array_equal(got[0]["all0_10_50_None"], got[0]["mask0_10_50_None"])
    assert not np.array_equal(got[0]["all0_10_50_None"], got[0][f"all0_10_50_{_floor()}"])
    r16 = got[1]["all0_16_400_None"]
    assert r16.shape[1] == 16 * 20
