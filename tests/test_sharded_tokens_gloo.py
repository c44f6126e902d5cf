"""CPU, world_size 2 over gloo: ``ShardedFlatIndex.set_tokens`` / ``get_tokens`` / ``search_maxsim`` / ``maxsim_ids`` and
the facade equal the unsharded numpy double (``tokens_fakes.FakeTokenIndex``), bit for bit.  Every component is a
multiple of 1/8, so every score is exact; a row's score is a function of its own matrix and of the query, so it has the
same bits wherever the row lives.  Covered: ``set_tokens`` in several global pieces that straddle the shard boundary,
several segments per shard, a shard without matrices, equal docs on both sides of the shard boundary (ties across it),
a truncating ``set_tokens``, an allow mask, tombstones, both metrics (larger first on either), fewer hits than ``k``,
ids in any order with repeats."""
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
KS = (1, 5, 16, 128)
QUERY_LENS = (1, 3, 17, 64)
TWINS = (5, 99, 100, 101, 250, 340)   # the same matrix on both shards: ties across the boundary at row 100


def _data():
    from claude_semantic_search_amd.late_interaction import bf16_to_f32, f32_to_bf16

    rng = np.random.default_rng(31)
    x = (rng.integers(-8, 9, size=(N, D_)) / 8.0).astype(np.float32)
    mats = [f32_to_bf16((rng.integers(-8, 9, size=(int(rng.integers(0, 7)), P)) / 8.0).astype(np.float32)) for _ in range(N)]
    qs = [f32_to_bf16((rng.integers(-8, 9, size=(m, P)) / 8.0).astype(np.float32)) for m in QUERY_LENS]
    for r in TWINS:                                     # sign(q) of query 2: no doc scores higher, so the twins lead its list
        mats[r] = f32_to_bf16(np.sign(bf16_to_f32(qs[2])).astype(np.float32))
    mats[3] = f32_to_bf16((rng.integers(-8, 9, size=(4, P)) / 8.0).astype(np.float32))
    mats[7] = np.zeros((0, P), np.uint16)
    return x, mats, qs


def _cat(res):
    return np.concatenate([a.astype(np.float64) for a in res], axis=1)


def _searches(ix, qs, out, tag, allow=None, ks=KS):
    ids = np.array([340, 0, 100, 99, 7, 100, 250, 199], np.int64)
    ids = ids[ids < (getattr(ix, "ntotal_global", None) or ix.ntotal)]
    for j, q in enumerate(qs):
        for k in ks:
            out[f"{tag}_s_{j}_{k}"] = _cat(ix.search_maxsim(q, k, allow=allow))
        out[f"{tag}_i_{j}"] = ix.maxsim_ids(q, ids).view(np.uint32).astype(np.float64)
    off, tok = ix.get_tokens()
    out[f"{tag}_off"], out[f"{tag}_tok"] = off.astype(np.float64), tok.astype(np.float64)


def _worker(rank, world, port, out_dir):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from claude_semantic_search_amd.sharded import ShardedFlatIndex, ShardedIndexFacade
        from related_fakes import merge_lists
        from tokens_fakes import FakeTokenIndex, Matrices

        x, mats, qs = _data()
        out = {}
        allow = (np.arange(N) % 4) != 1
        for metric in (0, 1):
            sh = ShardedFlatIndex(D_, metric, index_factory=lambda: FakeTokenIndex(D_, metric), merge=merge_lists(metric))
            sh.add_global(x[:200])                        # rank 0: rows 0..99, rank 1: rows 100..199
            _searches(sh, qs, out, f"none{metric}", ks=(16,))               # no matrix set yet
            sh.set_tokens(mats[:60])
            assert sh.token_rows == 60 and sh.token_dim == P and sh.local.token_rows == (60 if rank == 0 else 0)
            _searches(sh, qs, out, f"one{metric}", ks=(16, 128))            # rank 1 is a shard without matrices
            sh.set_tokens(Matrices.of(mats[60:140], P).csr, row0=60)        # the CSR form; straddles the shard boundary
            assert sh.token_rows == 140
            routed = [c for c in sh.local.calls if c[0] == "set_tokens"]
            assert routed == ([("set_tokens", 0, 60), ("set_tokens", 60, 40)] if rank == 0 else [("set_tokens", 0, 0), ("set_tokens", 0, 40)])
            _searches(sh, qs, out, f"part{metric}", ks=(16,))               # rows 140.. have no matrix
            sh.set_tokens(mats[140:200])
            sh.add_routed(x[200:241])
            sh.add_global(x[241:])
            assert len(sh.segments) >= 2
            sh.set_tokens(mats[200:300])
            sh.set_tokens(mats[250:], row0=250)           # drops the matrices of rows 250..299, then appends
            assert sh.token_rows == N and sh.local.token_rows == sh.shard_sizes[rank]
            _searches(sh, qs, out, f"all{metric}")
            _searches(sh, qs, out, f"mask{metric}", allow=allow, ks=(16,))
            sh.mark_deleted([0, 5, 150, 220, 340])
            _searches(sh, qs, out, f"dead{metric}", allow=allow, ks=(16,))
            sh.set_tokens(mats[:120], row0=0)             # the rewrite: rows 120.. lose their matrices
            _searches(sh, qs, out, f"cut{metric}", allow=allow, ks=(16,))
            sh.drop_tokens()
            assert sh.token_rows == 0 and sh.token_dim == 0 and sh.local.token_rows == 0
        fac = ShardedIndexFacade(D_, 0, index_factory=lambda: FakeTokenIndex(D_, 0), merge=merge_lists(0))
        for lo in range(0, N, 31):
            fac.add(x[lo:lo + 31])
        fac.set_tokens(mats)
        assert fac.token_rows == N and fac.token_dim == P
        _searches(fac, qs, out, "fac", ks=(16,))
        for call in (lambda: fac.search_maxsim(qs[0], 0), lambda: fac.search_maxsim(qs[0], 129),
                     lambda: fac.search_maxsim(np.zeros((65, P), np.uint16), 5), lambda: fac.search_maxsim(np.zeros((2, 48), np.uint16), 5),
                     lambda: fac.maxsim_ids(qs[0], [N]), lambda: fac.maxsim_ids(qs[0], [-1]),
                     lambda: fac.set_tokens(mats[:1], row0=N + 1), lambda: fac.set_tokens(mats[:1], row0=-1),
                     lambda: fac.set_tokens([np.zeros((2, 64), np.uint16)], row0=5),
                     lambda: fac.set_tokens([np.full((2, P), 0x7FC0, np.uint16)], row0=0)):
            try:
                call()
                raise AssertionError("a bad token call did not raise")
            except ValueError:
                pass
        np.savez(os.path.join(out_dir, f"p{rank}.npz"), **out)
    finally:
        dist.destroy_process_group()


def test_two_rank_maxsim_search_equals_the_unsharded_double(tmp_path):
    from tokens_fakes import FakeTokenIndex

    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    mp.spawn(_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    got = [np.load(tmp_path / f"p{r}.npz") for r in range(2)]
    x, mats, qs = _data()

    def whole(rows, row_mats, metric):
        ix = FakeTokenIndex(D_, metric)
        ix.add(rows)
        if row_mats:
            ix.set_tokens(row_mats)
        return ix

    allow = (np.arange(N) % 4) != 1
    dead = allow.copy()
    dead[[0, 5, 150, 220, 340]] = False
    for metric in (0, 1):
        want = {}
        _searches(whole(x[:200], [], metric), qs, want, f"none{metric}", ks=(16,))
        _searches(whole(x[:200], mats[:60], metric), qs, want, f"one{metric}", ks=(16, 128))
        _searches(whole(x[:200], mats[:140], metric), qs, want, f"part{metric}", ks=(16,))
        ix = whole(x, mats, metric)
        _searches(ix, qs, want, f"all{metric}")
        _searches(ix, qs, want, f"mask{metric}", allow=allow, ks=(16,))
        _searches(ix, qs, want, f"dead{metric}", allow=dead, ks=(16,))
        _searches(whole(x, mats[:120], metric), qs, want, f"cut{metric}", allow=dead, ks=(16,))
        if metric == 0:
            for key in [k for k in want if k.startswith("all0_") and (k.split("_")[-1] == "16" or k.split("_")[1] in ("i", "off", "tok"))]:
                want["fac_" + key[5:]] = want[key]
        for r in range(2):
            for key, val in want.items():
                assert got[r][key].shape == val.shape and np.array_equal(got[r][key], val), (key, r)
    # the cases are what they claim
    assert (got[0]["none0_s_0_16"][:, 16:] == -1).all() and (got[0]["none0_i_0"] == 0xFF800000).all()      # -inf bits
    ids = got[0]["all0_s_2_16"][:, 16:].astype(np.int64)
    assert (ids < 100).any() and (ids >= 100).any() and (ids >= 0).all()           # rows of both shards
    ids1 = got[0]["one0_s_2_16"][:, 16:].astype(np.int64)
    assert (ids1 < 60).all() and (ids1 >= 0).all()                                 # a shard without matrices returns nothing
    assert np.array_equal(got[0]["all0_s_1_16"], got[0]["all1_s_1_16"])            # the search does not see the metric
    # the twins tie across the shard boundary and come in id order
    ix = whole(x, mats, 0)
    col = ix._column(qs[2])
    assert len({float(col[r]) for r in TWINS}) == 1
    D, I = ix.search_maxsim(qs[2], 128)
    assert I[0, :len(TWINS)].tolist() == list(TWINS)
    assert got[1]["all0_s_2_128"][0, 128:128 + len(TWINS)].astype(np.int64).tolist() == list(TWINS)
    short = got[0]["one1_s_0_128"][:, 128:]
    assert (short >= 0).any() and (short == -1).any()                              # fewer hits than k
