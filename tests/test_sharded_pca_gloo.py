"""CPU, world_size 2 over gloo: ``ShardedFlatIndex.gram`` / ``pca`` / ``transform`` and the facade equal ONE numpy double
(``pca_fakes.FakePcaIndex``) that holds all rows -- Gram matrix, column sums, count, ``PcaResult`` and transformed rows
bit for bit, because every shard quantises under the GLOBAL shift and integers add up in any order.  Covered: several
segments per shard, one row far longer than the rest on one shard only (``e`` differs between the shards and the
global maximum decides the shift), an allow mask, tombstones, a row range across shards, and the facade."""
import os
import socket
import sys
from pathlib import Path

import numpy as np
import torch.distributed as dist
import torch.multiprocessing as mp

sys.path.insert(0, str(Path(__file__).resolve().parent))

D_ = 16
N = 413
DEAD = [3, 120, 250, 412]


def _data():
    from kmeans_fakes import planted

    x = planted(N, D_, 5, seed=33)[0]
    x[37] *= 16.0            # one long row (it lands on rank 0): the shift follows the GLOBAL maximum
    rng = np.random.default_rng(8)
    A = rng.standard_normal((3, D_)).astype(np.float32)
    b = rng.standard_normal(3).astype(np.float32)
    return x, A, b


def _pack(key, g, res, out):
    out[f"{key}_gram"], out[f"{key}_colsum"] = g.gram, g.colsum
    out[f"{key}_meta"] = np.array([g.count, g.shift, res.count, res.shift], np.int64)
    out[f"{key}_mean"], out[f"{key}_comp"], out[f"{key}_eig"] = res.mean, res.components, res.eigenvalues
    out[f"{key}_tv"] = np.array([res.total_variance])


def _worker(rank, world, port, out_dir):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from claude_semantic_search_amd.sharded import ShardedFlatIndex, ShardedIndexFacade
        from pca_fakes import FakePcaIndex
        from related_fakes import merge_lists

        x, A, b = _data()
        out = {}
        sh = ShardedFlatIndex(D_, 1, index_factory=lambda: FakePcaIndex(D_, 1), merge=merge_lists(1))
        sh.add_global(x[:200])
        sh.add_routed(x[200:241])
        sh.add_global(x[241:])
        assert len(sh.segments) >= 2
        out["e_local"] = np.array([sh.local.bounds()["max_norm2"], sh.local.ntotal])
        mask = (np.arange(N) % 3) == 0
        _pack("plain", sh.gram(), sh.pca(3), out)
        _pack("mask", sh.gram(allow=mask), sh.pca(2, allow=mask, whiten=True), out)
        _pack("low", sh.gram(fx_shift=5), sh.pca(1), out)
        out["y_all"] = sh.transform(A, b)
        out["y_part"] = sh.transform(A, None, row0=95, n=250)
        out["y_none"] = sh.transform(A[:1], b[:1], row0=7, n=0)
        sh.mark_deleted(DEAD)
        _pack("dead", sh.gram(), sh.pca(3), out)
        out["y_dead"] = sh.transform(A, b, row0=0, n=5)           # tombstoned rows are transformed like any other
        fac = ShardedIndexFacade(D_, 1, index_factory=lambda: FakePcaIndex(D_, 1), merge=merge_lists(1))
        for lo in range(0, N, 31):
            fac.add(x[lo:lo + 31])
        _pack("fac", fac.gram(), fac.pca(3), out)
        out["y_fac"] = fac.transform(A, b, row0=100)
        for bad in (dict(row0=N - 1, n=2), dict(row0=-1, n=1)):
            try:
                sh.transform(A, b, **bad)
                raise AssertionError("rows outside the index did not raise")
            except ValueError:
                pass
        try:
            sh.pca(2, allow=np.zeros(N, bool))
            raise AssertionError("a PCA of no rows did not raise")
        except ValueError:
            pass
        np.savez(os.path.join(out_dir, f"p{rank}.npz"), **out)
    finally:
        dist.destroy_process_group()


def test_two_rank_pca_equals_one_double_bit_for_bit(tmp_path):
    from claude_semantic_search_amd import flat_index as fi
    from pca_fakes import FakePcaIndex

    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    mp.spawn(_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    got = [np.load(tmp_path / f"p{r}.npz") for r in range(2)]
    x, A, b = _data()
    whole = FakePcaIndex(D_, 1)
    whole.add(x)
    mask = (np.arange(N) % 3) == 0
    live = np.ones(N, bool)
    live[DEAD] = False
    want = {}
    _pack("plain", whole.gram(), whole.pca(3), want)
    _pack("mask", whole.gram(allow=mask), whole.pca(2, allow=mask, whiten=True), want)
    g5 = whole.gram(fx_shift=5)
    _pack("low", g5, whole.pca(1), want)
    _pack("dead", whole.gram(allow=live), whole.pca(3, allow=live), want)
    _pack("fac", whole.gram(), whole.pca(3), want)
    want["y_all"] = whole.transform(A, b)
    want["y_part"] = whole.transform(A, None, 95, 250)
    want["y_none"] = np.zeros((0, 1), np.float32)
    want["y_dead"] = whole.transform(A, b, 0, 5)
    want["y_fac"] = whole.transform(A, b, 100)
    for r in range(2):
        for key, v in want.items():
            assert got[r][key].shape == np.asarray(v).shape and got[r][key].tobytes() == np.asarray(v).tobytes(), (key, r)
    # the cases are what they claim: the shards' own exponents differ, the long row moved the shift, the imposed shift
    # was used, the mask and the tombstones changed the integers
    e = [fi.pca_shift(float(got[r]["e_local"][0]), int(got[r]["e_local"][1]))[1] for r in range(2)]
    assert e[0] != e[1] and 0 < got[0]["e_local"][1] < N
    short = x.copy()
    short[37] /= 16.0
    n2 = lambda a: float((a.astype(np.float64) ** 2).sum(axis=1).max())   # noqa: E731
    assert want["plain_meta"][1] == fi.pca_shift(n2(x), N)[0] < fi.pca_shift(n2(short), N)[0]
    assert want["low_meta"][1] == 5 and not np.array_equal(want["low_gram"], want["plain_gram"])
    assert want["mask_meta"][0] == int(mask.sum()) and want["dead_meta"][0] == N - len(DEAD)
