"""CPU, world_size 2 over gloo: ``ShardedFlatIndex.range_search`` (local range search -> all-gather of the per-query
counts -> all-gather of the padded payload -> per-query merge) equals ONE unsharded index, for both metrics, with
several segments per shard, allow-masks and tombstones.  The local indexes are numpy doubles defined here (scores in
float32 from one formula, so the sharded and the unsharded double give the same bits)."""
import os
import socket

import numpy as np
import pytest
import torch.distributed as dist
import torch.multiprocessing as mp


def _scores(x, q, metric):
    x64, q64 = x.astype(np.float64), q.astype(np.float64)
    if metric == 0:
        return (q64 @ x64.T).astype(np.float32)
    return ((q64[:, None, :] - x64[None, :, :]) ** 2).sum(-1).astype(np.float32)


def _range(x, q, metric, radius, allow=None, base=0):
    """The contract of ``IndexFlat.range_search`` in numpy: strict, best first, ties by id."""
    s = _scores(x, q, metric) if x.shape[0] else np.zeros((q.shape[0], 0), np.float32)
    r = np.float32(radius)
    lims, D, I = [0], [np.empty(0, np.float32)], [np.empty(0, np.int64)]
    for j in range(q.shape[0]):
        hit = s[j] > r if metric == 0 else s[j] < r
        if allow is not None:
            hit = hit & np.asarray(allow, bool)
        ids = np.flatnonzero(hit)
        order = np.lexsort((ids, -s[j, ids] if metric == 0 else s[j, ids]))
        D.append(s[j, ids][order])
        I.append(ids[order].astype(np.int64) + base)
        lims.append(lims[-1] + ids.size)
    return np.array(lims, np.int64), np.concatenate(D), np.concatenate(I)


class _FakeLocal:
    def __init__(self, d, metric):
        self.d, self.metric, self.base = d, metric, 0
        self.x = np.zeros((0, d), np.float32)

    ntotal = property(lambda self: self.x.shape[0])

    def set_id_base(self, b):
        self.base = int(b)

    def reserve(self, n):
        pass

    def add(self, x, normalize=False):
        assert not normalize
        self.x = np.concatenate([self.x, np.asarray(x, np.float32)])

    def range_search(self, q, thresh, normalize=False, allow=None):
        assert not normalize
        return _range(self.x, np.asarray(q, np.float32), self.metric, thresh, allow, self.base)


D_, PARTS = 16, ((40, 61), (7, 62), (3, 63), (50, 64))      # (rows, seed) of the adds: global, routed, routed, global


def _data():
    from oracle import knn_oracle as ko

    x = ko.normalize_rows(np.concatenate([ko.synth_rows(n, D_, s) for n, s in PARTS]))
    q = ko.normalize_rows(ko.synth_rows(5, D_, 65))
    q[1] = x[3]            # a copy of a row of rank 0's first block: at a high radius only that row hits
    q[2] = x[95]           # ... and one of rank 1's last block
    return x, q


CASES = {0: (0.999, 0.3, -0.2, -2.0, 2.0), 1: (1e-6, 1.4, 2.4, 5.0, 0.0)}   # metric -> radii: one row .. everything .. nothing


def _worker(rank, world, port, out_dir):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from claude_semantic_search_amd.sharded import ShardedFlatIndex, ShardedIndexFacade

        x, q = _data()
        out = {}
        for metric in (0, 1):
            sh = ShardedFlatIndex(D_, metric, index_factory=lambda: _FakeLocal(D_, metric))
            r0 = 0
            for (n, _), how in zip(PARTS, ("global", "routed", "routed", "global")):
                (sh.add_global if how == "global" else sh.add_routed)(x[r0:r0 + n])
                r0 += n
            assert sh.ntotal_global == 100 and len(sh.segments) >= 2 and sh.local.ntotal == sh.shard_sizes[rank]
            for c, radius in enumerate(CASES[metric]):
                lims, D, I = sh.range_search(q, radius)
                out[f"m{metric}c{c}"] = (lims, D, I)
            allow = (np.arange(100) % 3) != 1
            out[f"m{metric}allow"] = sh.range_search(q, CASES[metric][2], allow=allow)
            sh.mark_deleted([3, 60, 99])
            out[f"m{metric}dead"] = sh.range_search(q, CASES[metric][2], allow=allow)
            out[f"m{metric}deadonly"] = sh.range_search(q[:0], CASES[metric][2])          # no queries
        fac = ShardedIndexFacade(D_, 0, index_factory=lambda: _FakeLocal(D_, 0))
        fac.add(x[:10])
        fac.add(x[10:30])
        out["facade"] = fac.range_search(q, 0.3)
        np.savez(os.path.join(out_dir, f"r{rank}.npz"), **{f"{k}_{n}": v for k, t in out.items() for n, v in zip("LDI", t)})
    finally:
        dist.destroy_process_group()


def test_two_rank_range_search_equals_one_index(tmp_path):
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    mp.spawn(_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    x, q = _data()
    got = [np.load(tmp_path / f"r{r}.npz") for r in range(2)]

    def same(key, want, what):
        for r in range(2):
            for n, w in zip("LDI", want):
                g = got[r][f"{key}_{n}"]
                assert g.dtype == w.dtype and np.array_equal(g, w), f"rank {r} {what}: {n} differs"

    for metric in (0, 1):
        for c, radius in enumerate(CASES[metric]):
            want = _range(x, q, metric, radius)
            same(f"m{metric}c{c}", want, f"metric {metric} radius {radius}")
        # the cases are what they claim: one hit from ONE rank only (the other sends nothing), unequal counts, all, none
        one = np.diff(_range(x, q, metric, CASES[metric][0])[0])
        assert one[1] == 1 and one[2] == 1 and one.sum() == 2
        assert np.array_equal(np.diff(_range(x, q, metric, CASES[metric][3])[0]), [100] * 5)
        assert _range(x, q, metric, CASES[metric][4])[0][-1] == 0
        mid = _range(x, q, metric, CASES[metric][2])
        assert 0 < mid[0][-1] < 500 and len(set(np.diff(mid[0]).tolist())) > 1
        allow = (np.arange(100) % 3) != 1
        same(f"m{metric}allow", _range(x, q, metric, CASES[metric][2], allow), "allow mask")
        dead = allow.copy()
        dead[[3, 60, 99]] = False
        same(f"m{metric}dead", _range(x, q, metric, CASES[metric][2], dead), "allow mask and tombstones")
        same(f"m{metric}deadonly", _range(x, q[:0], metric, 0.0), "no queries")
    same("facade", _range(x[:30], q, 0, 0.3), "facade")


def test_single_process_skips_the_exchange():
    """World 1 (no process group): the local result, ids through the segment table, no collective call."""
    from claude_semantic_search_amd.sharded import ShardedFlatIndex

    x, q = _data()
    sh = ShardedFlatIndex(D_, 0, index_factory=lambda: _FakeLocal(D_, 0))
    sh.add_global(x[:60])
    sh.add_routed(x[60:])
    lims, D, I = sh.range_search(q, 0.3)
    want = _range(x, q, 0, 0.3)
    assert np.array_equal(lims, want[0]) and np.array_equal(D, want[1]) and np.array_equal(I, want[2])
    with pytest.raises(ValueError):
        sh.range_search(q, 0.3, allow=np.ones(7, bool))
