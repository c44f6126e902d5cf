"""CPU, world_size 2 over gloo: ``ShardedFlatIndex`` / the facade with a token codec -- ``set_token_codec`` /
``set_tokens`` / ``set_token_codes`` / ``get_token_codes`` / ``get_tokens`` / ``search_maxsim`` / ``maxsim_ids`` -- equal ONE
unsharded numpy double (``tokens_codec_fakes.FakeCodecIndex``), bit for bit.  Lattice inputs (every component a
multiple of 1/8, lattice codec): every code, decoded value and score is exact; a row's codes and score are a function
of its own matrix, the codec and the query, so they have the same bits wherever the row lives.  Covered: pieces that
straddle the shard boundary, several segments per shard, a shard without matrices, a truncating rewrite, loading from
canonical codes, an allow mask, ids in any order with repeats."""
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
KS = (1, 16, 128)


def _data():
    import tokens_codec_cases as cc

    rng = np.random.default_rng(41)
    codec = cc.lattice_codec(P, 2, 17)
    x = (rng.integers(-8, 9, size=(N, D_)) / 8.0).astype(np.float32)
    mats = []
    for _ in range(N):
        m = int(rng.integers(0, 7))
        t = np.clip(codec.centroids[rng.integers(0, 17, size=m)] + rng.integers(-2, 3, size=(m, P)) / 8.0, -1.0, 1.0)
        mats.append(cc.to_bits(t.astype(np.float32)))
    for r in (99, 100, 250):                              # the same matrix on both shards: ties across the boundary
        mats[r] = mats[5]
    qs = [cc.to_bits((rng.integers(-8, 9, size=(m, P)) / 8.0).astype(np.float32)) for m in (1, 17, 64)]
    return codec, x, mats, qs


def _record(ix, qs, out, tag, allow=None, ks=KS):
    ids = np.array([340, 0, 100, 99, 7, 100, 250, 199], np.int64)
    ids = ids[ids < (getattr(ix, "ntotal_global", None) or ix.ntotal)]
    for j, q in enumerate(qs):
        for k in ks:
            D, I = ix.search_maxsim(q, k, allow=allow)
            out[f"{tag}_s_{j}_{k}"] = np.concatenate([D.astype(np.float64), I.astype(np.float64)], axis=1)
        out[f"{tag}_i_{j}"] = ix.maxsim_ids(q, ids).view(np.uint32).astype(np.float64)
    off, codes, res = ix.get_token_codes()
    out[f"{tag}_off"], out[f"{tag}_codes"], out[f"{tag}_res"] = off.astype(np.float64), codes.astype(np.float64), res.astype(np.float64)
    off, tok = ix.get_tokens()
    out[f"{tag}_toff"], out[f"{tag}_tok"] = off.astype(np.float64), tok.astype(np.float64)


def _worker(rank, world, port, out_dir):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from claude_semantic_search_amd.sharded import ShardedFlatIndex, ShardedIndexFacade
        from related_fakes import merge_lists
        from tokens_codec_fakes import FakeCodecIndex
        from tokens_fakes import Matrices

        codec, x, mats, qs = _data()
        out = {}
        allow = (np.arange(N) % 4) != 1
        sh = ShardedFlatIndex(D_, 0, index_factory=lambda: FakeCodecIndex(D_, 0), merge=merge_lists(0))
        sh.add_global(x[:200])                            # rank 0: rows 0..99, rank 1: rows 100..199
        assert sh.token_codec_bits == 0 and sh.get_token_codec() is None
        sh.set_token_codec(codec)                         # collective: every rank passes the same codec
        assert sh.token_codec_bits == 2 and sh.local.token_codec_bits == 2 and sh.get_token_codec().P == P
        sh.set_tokens(mats[:60])
        assert sh.token_rows == 60 and sh.token_dim == P and sh.local.token_rows == (60 if rank == 0 else 0)
        _record(sh, qs, out, "one", ks=(16,))             # rank 1 is a shard without matrices
        sh.set_tokens(Matrices.of(mats[60:140], P).csr, row0=60)   # straddles the shard boundary
        routed = [c for c in sh.local.calls if c[0] == "set_tokens"]
        assert routed == ([("set_tokens", 0, 60), ("set_tokens", 60, 40)] if rank == 0 else [("set_tokens", 0, 0), ("set_tokens", 0, 40)])
        sh.set_tokens(mats[140:200])
        sh.add_routed(x[200:241])
        sh.add_global(x[241:])
        assert len(sh.segments) >= 2
        sh.set_tokens(mats[200:300])
        sh.set_tokens(mats[250:], row0=250)               # drops the matrices of rows 250..299, then appends
        assert sh.token_rows == N and sh.local.token_rows == sh.shard_sizes[rank]
        _record(sh, qs, out, "all")
        _record(sh, qs, out, "mask", allow=allow, ks=(16,))
        saved = sh.get_token_codes()
        sh.set_tokens(mats[:120], row0=0)                 # the rewrite: rows 120.. lose their matrices
        _record(sh, qs, out, "cut", ks=(16,))
        sh.drop_tokens()
        assert sh.token_rows == 0 and sh.token_codec_bits == 2                   # the codec stays
        sh.set_token_codes(saved[0][:201], saved[1][:saved[0][200]], saved[2][:saved[0][200]])   # load from codes, in two pieces
        sh.set_token_codes(saved[0][200:] - saved[0][200], saved[1][saved[0][200]:], saved[2][saved[0][200]:])
        assert sh.token_rows == N and sh.token_dim == P
        assert [c for c in sh.local.calls if c[0] == "set_token_codes"]
        _record(sh, qs, out, "load", ks=(16,))
        fac = ShardedIndexFacade(D_, 0, index_factory=lambda: FakeCodecIndex(D_, 0), merge=merge_lists(0))
        for lo in range(0, N, 31):
            fac.add(x[lo:lo + 31])
        fac.set_token_codec(codec)
        fac.set_tokens(mats)
        assert fac.token_rows == N and fac.token_codec_bits == 2 and fac.get_token_codec().nbits == 2
        _record(fac, qs, out, "fac", ks=(16,))
        bad = saved[1].copy()
        bad[3] = 17
        for call in (lambda: fac.set_token_codes(saved[0], bad, saved[2], row0=0),
                     lambda: fac.set_token_codes(saved[0][:2], saved[1][:saved[0][1]], saved[2][:saved[0][1]], row0=N + 1),
                     lambda: fac.set_tokens([np.zeros((2, 64), np.uint16)], row0=5)):
            try:
                call()
                raise AssertionError("a bad call did not raise")
            except (ValueError, AssertionError) as e:
                assert "did not raise" not in str(e)
        np.savez(os.path.join(out_dir, f"p{rank}.npz"), **out)
    finally:
        dist.destroy_process_group()


def test_two_rank_compressed_token_matrices_equal_one_index(tmp_path):
    from tokens_codec_fakes import FakeCodecIndex

    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    mp.spawn(_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    got = [np.load(tmp_path / f"p{r}.npz") for r in range(2)]
    codec, x, mats, qs = _data()

    def whole(rows, row_mats):
        ix = FakeCodecIndex(D_, 0)
        ix.add(rows)
        ix.set_token_codec(codec)
        ix.set_tokens(row_mats)
        return ix

    allow = (np.arange(N) % 4) != 1
    want = {}
    _record(whole(x[:200], mats[:60]), qs, want, "one", ks=(16,))
    ix = whole(x, mats)
    _record(ix, qs, want, "all")
    _record(ix, qs, want, "mask", allow=allow, ks=(16,))
    _record(whole(x, mats[:120]), qs, want, "cut", ks=(16,))
    for key in [k for k in want if k.startswith("all_") and not k.endswith(("_1", "_128"))]:
        want["load_" + key[4:]] = want["fac_" + key[4:]] = want[key]
    for r in range(2):
        for key, val in want.items():
            assert got[r][key].shape == val.shape and np.array_equal(got[r][key], val), (key, r)
    # the cases are what they claim
    ids = got[0]["all_s_1_16"][:, 16:].astype(np.int64)
    assert (ids < 100).any() and (ids >= 100).any() and (ids >= 0).all()           # rows of both shards
    assert (got[0]["one_s_1_16"][:, 16:] < 60).all()                                # a shard without matrices returns nothing
    col = ix._column(qs[1])
    assert len({float(col[r]) for r in (5, 99, 100, 250)}) == 1                     # the twins tie across the boundary
    assert got[1]["all_codes"].shape[0] == sum(m.shape[0] for m in mats) and got[1]["all_res"].shape[1] == P * 2 // 8
    # ... and the double's decoded matrices differ from the stored ones: the searches ran on the codes
    from tokens_fakes import Matrices
    assert not np.array_equal(got[0]["all_tok"], Matrices.of(mats, P).tok.astype(np.float64))
