"""CPU, world_size 2 over gloo: ``ShardedFlatIndex.search_maxsim_batch`` and the facade equal the unsharded numpy double
(``tokens_batch_fakes.FakeTokenBatchIndex``, the loop of single calls), bit for bit, masks included.  The data are
those of tests/test_sharded_tokens_gloo.py: lattice components, twins on both sides of the shard boundary."""
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
KS = (1, 16, 128)
ORDER = (2, 0, 3, 1, 2, 2, 0, 3, 1, 3, 0)   # 11 queries: equal ones in different places


def _batch(qs):
    return [qs[i] for i in ORDER]


def _cat(res):
    return np.concatenate([a.astype(np.float64) for a in res], axis=1)


def _searches(ix, qs, out, tag, allow=None):
    for k in KS:
        out[f"{tag}_{k}"] = _cat(ix.search_maxsim_batch(_batch(qs), k, allow=allow))


def _worker(rank, world, port, out_dir):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from claude_semantic_search_amd.sharded import ShardedFlatIndex, ShardedIndexFacade
        from related_fakes import merge_lists
        from tokens_batch_fakes import FakeTokenBatchIndex

        x, mats, qs = base._data()
        out = {}
        allow = (np.arange(N) % 4) != 1
        for metric in (0, 1):
            sh = ShardedFlatIndex(D_, metric, index_factory=lambda: FakeTokenBatchIndex(D_, metric), merge=merge_lists(metric))
            sh.add_global(x[:200])
            _searches(sh, qs, out, f"none{metric}")                            # no matrix set yet
            sh.set_tokens(mats[:60])
            _searches(sh, qs, out, f"one{metric}")                             # rank 1 is a shard without matrices
            sh.set_tokens(mats[60:200])
            sh.add_routed(x[200:241])
            sh.add_global(x[241:])
            sh.set_tokens(mats[200:])
            _searches(sh, qs, out, f"all{metric}")
            _searches(sh, qs, out, f"mask{metric}", allow=allow)
            assert [c for c in sh.local.calls if c[0] == "search_maxsim_batch"][-1] == ("search_maxsim_batch", len(ORDER), 128, True)
        fac = ShardedIndexFacade(D_, 0, index_factory=lambda: FakeTokenBatchIndex(D_, 0), merge=merge_lists(0))
        for lo in range(0, N, 31):
            fac.add(x[lo:lo + 31])
        fac.set_tokens(mats)
        _searches(fac, qs, out, "fac", allow=allow)
        for call in (lambda: fac.search_maxsim_batch([], 5), lambda: fac.search_maxsim_batch(_batch(qs), 129),
                     lambda: fac.search_maxsim_batch([qs[0], np.zeros((65, P), np.uint16)], 5),
                     lambda: fac.search_maxsim_batch([qs[0], np.zeros((2, 64), np.uint16)], 5)):
            try:
                call()
                raise AssertionError("a bad batch call did not raise")
            except ValueError:
                pass
        np.savez(os.path.join(out_dir, f"p{rank}.npz"), **out)
    finally:
        dist.destroy_process_group()


def test_two_rank_batched_maxsim_search_equals_the_unsharded_double(tmp_path):
    from tokens_batch_fakes import FakeTokenBatchIndex

    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    mp.spawn(_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    got = [np.load(tmp_path / f"p{r}.npz") for r in range(2)]
    x, mats, qs = base._data()

    def whole(rows, row_mats, metric):
        ix = FakeTokenBatchIndex(D_, metric)
        ix.add(rows)
        if row_mats:
            ix.set_tokens(row_mats)
        return ix

    allow = (np.arange(N) % 4) != 1
    for metric in (0, 1):
        want = {}
        _searches(whole(x[:200], [], metric), qs, want, f"none{metric}")
        _searches(whole(x[:200], mats[:60], metric), qs, want, f"one{metric}")
        ix = whole(x, mats, metric)
        _searches(ix, qs, want, f"all{metric}")
        _searches(ix, qs, want, f"mask{metric}", allow=allow)
        if metric == 0:
            _searches(ix, qs, want, "fac", allow=allow)
        for r in range(2):
            for key, val in want.items():
                assert got[r][key].shape == val.shape and np.array_equal(got[r][key], val), (key, r)
        # ... and the double's rows are the single calls'
        for b, i in enumerate(ORDER):
            assert np.array_equal(want[f"mask{metric}_16"][b:b + 1], _cat(ix.search_maxsim(qs[i], 16, allow=allow)))
    # the cases are what they claim
    assert (got[0]["none0_16"][:, 16:] == -1).all()
    ids = got[0]["all0_16"][:, 16:].astype(np.int64)
    assert (ids < 100).any() and (ids >= 100).any()                                # rows of both shards
    assert np.array_equal(got[1]["all0_128"][0], got[1]["all0_128"][4])            # equal queries, equal rows
    assert not np.array_equal(got[1]["all0_128"][0], got[1]["all0_128"][1])
    assert got[1]["all0_128"][0, 128:128 + len(base.TWINS)].astype(np.int64).tolist() == list(base.TWINS)
    assert not np.array_equal(got[0]["all0_16"], got[0]["mask0_16"])
