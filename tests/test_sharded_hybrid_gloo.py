"""CPU, world_size 2 over gloo: ``ShardedFlatIndex.set_terms`` / ``term_stats`` / ``search_hybrid`` and the facade equal
the unsharded numpy double (``lexical_fakes.FakeLexIndex``), ``(D, I, S, L)`` bit for bit and the statistics exactly.
Rows and queries are multiples of 1/8, so every dense score is exact; the lexical value of a row is a function of its
own list and of the call's weights and constants, which every shard receives alike (``avgdl`` from the GLOBAL
statistics).  Covered: ``set_terms`` in several global pieces that straddle the shard boundary, several segments per
shard, rows without lists, a truncating ``set_terms``, an allow mask, tombstones, both metrics."""
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
ALPHAS = (0.5, 2.0)
QUERIES = ((3, 17, 5), (0,), (23, 1, 2, 9, 11), ())
STAT_TERMS = list(range(V)) + [1000]


def _data():
    rng = np.random.default_rng(23)
    q = (rng.integers(-8, 9, size=(len(QUERIES), D_)) / 8.0).astype(np.float32)
    x = (rng.integers(-8, 9, size=(N, D_)) / 8.0).astype(np.float32)
    lists = [np.floor(V * rng.random(int(rng.integers(0, 12))) ** 2).astype(np.int64) for _ in range(N)]
    return q, x, lists


def _weights(ix, terms):
    from claude_semantic_search_amd.lexical import bm25_weights

    df, n, _ = ix.term_stats(terms)
    return bm25_weights(df, n)


def _cat(res):
    return np.concatenate([a.astype(np.float64) for a in res], axis=1)


def _stats(ix):
    df, n, total = ix.term_stats(STAT_TERMS)
    return np.concatenate([np.asarray(df, np.int64), [n, total]])


def _searches(ix, q, out, tag, allow=None, ks=KS):
    for j, terms in enumerate(QUERIES):
        w = _weights(ix, terms)
        for k in ks:
            for a in ALPHAS:
                out[f"{tag}_{j}_{k}_{a}"] = _cat(ix.search_hybrid(q[j], terms, w, k, a, allow=allow))


def _worker(rank, world, port, out_dir):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from claude_semantic_search_amd.sharded import ShardedFlatIndex, ShardedIndexFacade
        from lexical_fakes import FakeLexIndex
        from related_fakes import merge_lists

        q, x, lists = _data()
        out = {}
        allow = (np.arange(N) % 4) != 1
        for metric in (0, 1):
            sh = ShardedFlatIndex(D_, metric, index_factory=lambda: FakeLexIndex(D_, metric), merge=merge_lists(metric))
            sh.add_global(x[:200])                        # rank 0: rows 0..99, rank 1: rows 100..199
            out[f"nostat{metric}"] = _stats(sh)
            _searches(sh, q, out, f"none{metric}", ks=(16,))                # no list set yet
            sh.set_terms(lists[:60])                      # three global pieces; the second straddles the shard boundary
            sh.set_terms(lists[60:140], row0=60)
            out[f"partstat{metric}"] = _stats(sh)
            _searches(sh, q, out, f"part{metric}", ks=(16,))                # rows 140.. have no list
            sh.set_terms(lists[140:200])
            sh.add_routed(x[200:241])
            sh.add_global(x[241:])
            assert len(sh.segments) >= 2
            sh.set_terms(lists[200:300])
            sh.set_terms(lists[250:], row0=250)           # truncates the lists of rows 250..299, then appends
            out[f"allstat{metric}"] = _stats(sh)
            _searches(sh, q, out, f"all{metric}")
            _searches(sh, q, out, f"mask{metric}", allow=allow, ks=(16,))
            sh.mark_deleted([0, 7, 150, 220, 340])
            _searches(sh, q, out, f"dead{metric}", allow=allow, ks=(16,))
            sh.set_terms(lists[:120], row0=0)             # the rewrite: rows 120.. lose their lists
            out[f"cutstat{metric}"] = _stats(sh)
        fac = ShardedIndexFacade(D_, 0, index_factory=lambda: FakeLexIndex(D_, 0), merge=merge_lists(0))
        for lo in range(0, N, 31):
            fac.add(x[lo:lo + 31])
        fac.set_terms(lists)
        out["facstat"] = _stats(fac)
        _searches(fac, q, out, "fac", ks=(16,))
        w = _weights(fac, QUERIES[0])
        for bad in (dict(k=0), dict(k=129), dict(alpha=float("nan")), dict(terms=(3, 3, 5)), dict(avgdl=0.0)):
            args = dict(terms=QUERIES[0], k=5, alpha=0.5)
            args.update(bad)
            try:
                fac.search_hybrid(q[0], args.pop("terms"), w, args.pop("k"), args.pop("alpha"), **args)
                raise AssertionError(f"search_hybrid({bad}) did not raise")
            except ValueError:
                pass
        for row0 in (N + 1, -1):
            try:
                fac.set_terms(lists[:1], row0=row0)
                raise AssertionError("set_terms beyond the rows did not raise")
            except ValueError:
                pass
        np.savez(os.path.join(out_dir, f"p{rank}.npz"), **out)
    finally:
        dist.destroy_process_group()


def test_two_rank_hybrid_search_equals_the_unsharded_double(tmp_path):
    from lexical_fakes import FakeLexIndex

    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    mp.spawn(_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    got = [np.load(tmp_path / f"p{r}.npz") for r in range(2)]
    q, x, lists = _data()

    def whole(rows, row_lists, metric):
        ix = FakeLexIndex(D_, metric)
        ix.add(rows)
        if row_lists:
            ix.set_terms(row_lists)
        return ix

    allow = (np.arange(N) % 4) != 1
    dead = allow.copy()
    dead[[0, 7, 150, 220, 340]] = False
    for metric in (0, 1):
        want = {}
        ix = whole(x[:200], [], metric)
        want[f"nostat{metric}"] = _stats(ix)
        _searches(ix, q, want, f"none{metric}", ks=(16,))
        ix = whole(x[:200], lists[:140], metric)
        want[f"partstat{metric}"] = _stats(ix)
        _searches(ix, q, want, f"part{metric}", ks=(16,))
        ix = whole(x, lists, metric)
        want[f"allstat{metric}"] = _stats(ix)
        _searches(ix, q, want, f"all{metric}")
        _searches(ix, q, want, f"mask{metric}", allow=allow, ks=(16,))
        _searches(ix, q, want, f"dead{metric}", allow=dead, ks=(16,))
        want[f"cutstat{metric}"] = _stats(whole(x, lists[:120], metric))
        if metric == 0:
            want["facstat"] = want["allstat0"]
            for key in [k for k in want if k.startswith("all0_") and k.split("_")[2] == "16"]:
                want["fac_" + key[5:]] = want[key]
        for r in range(2):
            for key, val in want.items():
                assert np.array_equal(got[r][key], val), (key, r)
    # the cases are what they claim: lists change the answer, rows of both shards are in it, statistics are not trivial
    assert not np.array_equal(got[0]["part0_0_16_2.0"], got[0]["none0_0_16_2.0"])
    ids = got[0]["all0_0_16_2.0"][:, 16:32].astype(np.int64)
    assert (ids < 100).any() and (ids >= 100).any()
    assert got[0]["nostat0"][:-2].sum() == 0 and got[0]["nostat0"][-1] == 0 and got[0]["nostat0"][-2] == 200
    assert got[0]["allstat0"][-1] == sum(len(l) for l in lists) and got[0]["allstat0"][-2] == N
    assert got[0]["cutstat0"][-1] == sum(len(l) for l in lists[:120])
    L = got[0]["all0_0_16_2.0"][:, 48:]
    assert (L > 0).any()
