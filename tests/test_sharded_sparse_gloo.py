"""CPU, world_size 2 over gloo: ``ShardedFlatIndex.set_sparse`` / ``search_sparse`` / ``search_hybrid_sparse`` and the
facade equal the unsharded numpy double (``sparse_fakes.FakeSparseIndex``), ``(D, I)`` and ``(D, I, S, L)`` bit for bit.
Rows, queries and every sparse weight are multiples of 1/8, so every value is exact; a row's dot product is a function
of its own vector and of the query, with no corpus statistics, so it has the same bits wherever the row lives.  Covered:
``set_sparse`` in several global pieces that straddle the shard boundary, several segments per shard, rows without
vectors, a truncating ``set_sparse``, an allow mask, tombstones, both metrics (the pure search ranks larger-first on
either), negative query weights, fewer hits than ``k``."""
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
V = 24
KS = (1, 5, 16, 128)
ALPHA = 0.5
QUERIES = (((3, 17, 5), (1.0, 0.5, 2.0)), ((23,), (0.25,)), ((23, 1, 2, 9, 11), (1.5, -0.5, 0.125, -2.0, 4.0)), ((), ()),
           ((1000,), (1.0,)))


def _data():
    rng = np.random.default_rng(29)
    q = (rng.integers(-8, 9, size=(len(QUERIES), D_)) / 8.0).astype(np.float32)
    x = (rng.integers(-8, 9, size=(N, D_)) / 8.0).astype(np.float32)
    vectors = []
    for _ in range(N):
        t = np.unique(np.floor(V * rng.random(int(rng.integers(0, 9))) ** 2).astype(np.int64))
        vectors.append((rng.permutation(t), (rng.integers(1, 33, size=t.shape[0]) / 8.0).astype(np.float32)))
    return q, x, vectors


def _cat(res):
    return np.concatenate([a.astype(np.float64) for a in res], axis=1)


def _searches(ix, q, out, tag, allow=None, ks=KS):
    for j, (terms, weights) in enumerate(QUERIES):
        for k in ks:
            out[f"{tag}_s_{j}_{k}"] = _cat(ix.search_sparse(terms, weights, k, allow=allow))
            out[f"{tag}_h_{j}_{k}"] = _cat(ix.search_hybrid_sparse(q[j], terms, weights, k, ALPHA, allow=allow))


def _worker(rank, world, port, out_dir):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from claude_semantic_search_amd.sharded import ShardedFlatIndex, ShardedIndexFacade
        from related_fakes import merge_lists
        from sparse_fakes import FakeSparseIndex

        q, x, vectors = _data()
        out = {}
        allow = (np.arange(N) % 4) != 1
        for metric in (0, 1):
            sh = ShardedFlatIndex(D_, metric, index_factory=lambda: FakeSparseIndex(D_, metric), merge=merge_lists(metric))
            sh.add_global(x[:200])                        # rank 0: rows 0..99, rank 1: rows 100..199
            _searches(sh, q, out, f"none{metric}", ks=(16,))                # no vector set yet
            sh.set_sparse(vectors[:60])                   # three global pieces; the second straddles the shard boundary
            sh.set_sparse(vectors[60:140], row0=60)
            assert sh.sparse_rows == 140
            routed = [c for c in sh.local.calls if c[0] == "set_sparse"]
            # routing through the segment table: rank 0 got local rows [0, 60) then [60, 100), rank 1 nothing then [0, 40)
            assert routed == ([("set_sparse", 0, 60), ("set_sparse", 60, 40)] if rank == 0 else [("set_sparse", 0, 0), ("set_sparse", 0, 40)])
            _searches(sh, q, out, f"part{metric}", ks=(16,))                # rows 140.. have no vector
            sh.set_sparse(vectors[140:200])
            sh.add_routed(x[200:241])
            sh.add_global(x[241:])
            assert len(sh.segments) >= 2
            sh.set_sparse(vectors[200:300])
            sh.set_sparse(vectors[250:], row0=250)        # drops the vectors of rows 250..299, then appends
            assert sh.sparse_rows == N and sh.local.sparse_rows == sh.shard_sizes[rank]
            _searches(sh, q, out, f"all{metric}")
            _searches(sh, q, out, f"mask{metric}", allow=allow, ks=(16,))
            sh.mark_deleted([0, 7, 150, 220, 340])
            _searches(sh, q, out, f"dead{metric}", allow=allow, ks=(16,))
            sh.set_sparse(vectors[:120], row0=0)          # the rewrite: rows 120.. lose their vectors
            _searches(sh, q, out, f"cut{metric}", allow=allow, ks=(16,))
        fac = ShardedIndexFacade(D_, 0, index_factory=lambda: FakeSparseIndex(D_, 0), merge=merge_lists(0))
        for lo in range(0, N, 31):
            fac.add(x[lo:lo + 31])
        off = np.concatenate([[0], np.cumsum([len(t) for t, _ in vectors])]).astype(np.int64)
        fac.set_sparse((off, np.concatenate([t for t, _ in vectors]), np.concatenate([w for _, w in vectors])))   # the CSR form
        assert fac.sparse_rows == N
        _searches(fac, q, out, "fac", ks=(16,))
        for bad in (dict(k=0), dict(k=129), dict(terms=(3, 3, 5)), dict(weights=(1.0, 0.0, 1.0)), dict(weights=(1.0, float("nan"), 1.0)),
                    dict(terms=tuple(range(65)), weights=(1.0,) * 65)):
            args = dict(terms=QUERIES[0][0], weights=QUERIES[0][1], k=5)
            args.update(bad)
            for call in (lambda: fac.search_sparse(args["terms"], args["weights"], args["k"]),
                         lambda: fac.search_hybrid_sparse(q[0], args["terms"], args["weights"], args["k"], ALPHA)):
                try:
                    call()
                    raise AssertionError(f"a sparse search with {bad} did not raise")
                except ValueError:
                    pass
        for call in (lambda: fac.search_hybrid_sparse(q[0], (3,), (1.0,), 5, float("nan")),
                     lambda: fac.search_hybrid_sparse(q[:2], (3,), (1.0,), 5, ALPHA),
                     lambda: fac.set_sparse(vectors[:1], row0=N + 1), lambda: fac.set_sparse(vectors[:1], row0=-1),
                     lambda: fac.set_sparse([([3, 3], [1.0, 1.0])], row0=0), lambda: fac.set_sparse([([3], [0.0])], row0=0)):
            try:
                call()
                raise AssertionError("a bad sparse call did not raise")
            except ValueError:
                pass
        np.savez(os.path.join(out_dir, f"p{rank}.npz"), **out)
    finally:
        dist.destroy_process_group()


def test_two_rank_sparse_search_equals_the_unsharded_double(tmp_path):
    from sparse_fakes import FakeSparseIndex

    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    mp.spawn(_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    got = [np.load(tmp_path / f"p{r}.npz") for r in range(2)]
    q, x, vectors = _data()

    def whole(rows, row_vectors, metric):
        ix = FakeSparseIndex(D_, metric)
        ix.add(rows)
        if row_vectors:
            ix.set_sparse(row_vectors)
        return ix

    allow = (np.arange(N) % 4) != 1
    dead = allow.copy()
    dead[[0, 7, 150, 220, 340]] = False
    for metric in (0, 1):
        want = {}
        _searches(whole(x[:200], [], metric), q, want, f"none{metric}", ks=(16,))
        _searches(whole(x[:200], vectors[:140], metric), q, want, f"part{metric}", ks=(16,))
        ix = whole(x, vectors, metric)
        _searches(ix, q, want, f"all{metric}")
        _searches(ix, q, want, f"mask{metric}", allow=allow, ks=(16,))
        _searches(ix, q, want, f"dead{metric}", allow=dead, ks=(16,))
        _searches(whole(x, vectors[:120], metric), q, want, f"cut{metric}", allow=dead, ks=(16,))
        if metric == 0:
            for key in [k for k in want if k.startswith("all0_") and k.split("_")[3] == "16"]:
                want["fac_" + key[5:]] = want[key]
        for r in range(2):
            for key, val in want.items():
                assert np.array_equal(got[r][key], val), (key, r)
    # the cases are what they claim: vectors change the answer, rows of both shards are in it, short and empty answers occur
    assert not np.array_equal(got[0]["part0_h_0_16"], got[0]["none0_h_0_16"])
    ids = got[0]["all0_s_0_16"][:, 16:].astype(np.int64)
    assert (ids < 100).any() and (ids >= 100).any() and (ids >= 0).all()
    assert (got[0]["none0_s_0_16"][:, 16:] == -1).all() and (got[0]["all0_s_3_16"][:, 16:] == -1).all()
    assert (got[0]["all1_s_4_128"][:, 128:] == -1).all()                         # a term no row stores
    short = got[0]["all1_s_1_128"][:, 128:]
    assert (short >= 0).any() and (short == -1).any()                            # fewer hits than k
    D = got[0]["all1_s_2_128"][0, :128]
    assert (np.diff(D[got[0]["all1_s_2_128"][0, 128:] >= 0]) <= 0).all()         # larger first on an L2 index
    assert np.array_equal(got[0]["all0_s_2_16"], got[0]["all1_s_2_16"])          # the pure search does not see the metric
    assert (got[0]["all0_h_0_16"][:, 48:] > 0).any()                             # L
