"""CPU, world_size 2 and 3 over gloo: ``ShardedFlatIndex`` / the facade ``maxsim_candidates`` / ``search_maxsim_pruned``
equal ONE unsharded numpy double (``tokens_prune_fakes.FakePruneIndex``), bit for bit.  Lattice inputs: every
approximate and exact score is exact, and copies of one matrix on several shards tie on both, so the ``ncand`` cut and
the ``k`` cut both fall inside ties that straddle the shard boundaries.  Covered: several segments per shard, an allow
mask, ``ncand`` below, at and above the number of rows with tokens."""
import os
import socket
import sys
from pathlib import Path

import numpy as np
import torch.distributed as dist
import torch.multiprocessing as mp

sys.path.insert(0, str(Path(__file__).resolve().parent))

D_ = 8
N = 341
P = 32
NCANDS = (1, 7, 16, 100, 341, 65536)
TWINS = (5, 99, 100, 113, 114, 227, 250, 340)


def _data():
    import tokens_codec_cases as cc

    rng = np.random.default_rng(43)
    codec = cc.lattice_codec(P, 2, 17)
    x = (rng.integers(-8, 9, size=(N, D_)) / 8.0).astype(np.float32)
    pool = []
    for _ in range(40):                                   # 40 distinct matrices behind 341 rows: ties everywhere
        m = int(rng.integers(0, 7))
        t = np.clip(codec.centroids[rng.integers(0, 17, size=m)] + rng.integers(-2, 3, size=(m, P)) / 8.0, -1.0, 1.0)
        pool.append(cc.to_bits(t.astype(np.float32)))
    mats = [pool[int(i)] for i in rng.integers(0, 40, size=N)]
    big = cc.to_bits(np.clip(codec.centroids[np.arange(17)], -1.0, 1.0))     # every centroid: the best approximate score
    for r in TWINS:
        mats[r] = big
    qs = [cc.to_bits((rng.integers(-8, 9, size=(m, P)) / 8.0).astype(np.float32)) for m in (1, 17, 64)]
    return codec, x, mats, qs


def _record(ix, qs, out, tag, allow=None):
    for j, q in enumerate(qs):
        for ncand in NCANDS:
            ids, a = ix.maxsim_candidates(q, ncand, allow=allow)
            out[f"{tag}_c_{j}_{ncand}"] = np.concatenate([ids.astype(np.float64), a.view(np.uint32).astype(np.float64)])
            for k in (1, 16):
                if k <= ncand:
                    D, I = ix.search_maxsim_pruned(q, k, ncand, allow=allow)
                    out[f"{tag}_s_{j}_{ncand}_{k}"] = np.concatenate([D.view(np.uint32).astype(np.float64), I.astype(np.float64)], axis=1)


def _worker(rank, world, port, out_dir):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from claude_semantic_search_amd.sharded import ShardedFlatIndex, ShardedIndexFacade
        from related_fakes import merge_lists
        from tokens_prune_fakes import FakePruneIndex

        codec, x, mats, qs = _data()
        out = {}
        allow = (np.arange(N) % 4) != 1
        sh = ShardedFlatIndex(D_, 0, index_factory=lambda: FakePruneIndex(D_, 0), merge=merge_lists(0))
        sh.add_global(x[:200])
        sh.set_token_codec(codec)
        sh.add_routed(x[200:241])
        sh.add_global(x[241:])
        assert len(sh.segments) >= 2
        sh.set_tokens(mats)
        _record(sh, qs, out, "all")
        _record(sh, qs, out, "mask", allow=allow)
        assert [c for c in sh.local.calls if c[0] == "maxsim_candidates"] and [c for c in sh.local.calls if c[0] == "maxsim_ids"]
        fac = ShardedIndexFacade(D_, 0, index_factory=lambda: FakePruneIndex(D_, 0), merge=merge_lists(0))
        for lo in range(0, N, 31):
            fac.add(x[lo:lo + 31])
        fac.set_token_codec(codec)
        fac.set_tokens(mats)
        _record(fac, qs, out, "fac")
        for call in (lambda: sh.maxsim_candidates(qs[0], 0), lambda: sh.search_maxsim_pruned(qs[0], 17, 16),
                     lambda: fac.search_maxsim_pruned(qs[0], 0, 16)):
            try:
                call()
                raise AssertionError("a bad call did not raise")
            except ValueError:
                pass
        np.savez(os.path.join(out_dir, f"p{rank}.npz"), **out)
    finally:
        dist.destroy_process_group()


def _run(world, tmp_path):
    from tokens_prune_fakes import FakePruneIndex

    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    mp.spawn(_worker, args=(world, port, str(tmp_path)), nprocs=world, join=True)
    got = [np.load(tmp_path / f"p{r}.npz") for r in range(world)]
    codec, x, mats, qs = _data()
    ix = FakePruneIndex(D_, 0)
    ix.add(x)
    ix.set_token_codec(codec)
    ix.set_tokens(mats)
    allow = (np.arange(N) % 4) != 1
    want = {}
    _record(ix, qs, want, "all")
    _record(ix, qs, want, "mask", allow=allow)
    for key in [k for k in want if k.startswith("all_")]:
        want["fac_" + key[4:]] = want[key]
    for r in range(world):
        for key, val in want.items():
            assert got[r][key].shape == val.shape and np.array_equal(got[r][key], val), (key, r, world)
    # the cases are what they claim: the twins tie on the approximate AND the exact score, live on every shard, and the
    # cuts at ncand = 1 and 7 (of 8 twins) and at k = 1 fall inside them
    a, col = ix._approx(qs[1]), ix._column(qs[1])
    assert len({float(a[r]) for r in TWINS}) == 1 and len({float(col[r]) for r in TWINS}) == 1
    assert (a[list(TWINS)] >= a.max()).all()
    top = np.flatnonzero(a == a.max())
    assert top.size >= 8 and (top < N // world).any() and (top >= N - N // world).any()
    ids7 = want["all_c_1_7"][:7].astype(np.int64)
    assert np.array_equal(ids7, top[:7])
    live = int((a > -np.inf).sum())
    assert 100 < live < 341
    assert want["all_c_1_341"].shape[0] == 2 * live and want["all_c_1_100"].shape[0] == 200


def test_two_rank_candidates_and_pruned_search_equal_one_index(tmp_path):
    _run(2, tmp_path)


def test_three_rank_candidates_and_pruned_search_equal_one_index(tmp_path):
    _run(3, tmp_path)
