"""CPU, world_size 2 over gloo: ``ShardedFlatIndex.facets`` and the facade equal the unsharded numpy double
(``facets_fakes.FakeFacetIndex``) byte for byte -- counts, best scores, best GLOBAL ids, totals and unbucketed.  Rows
are multiples of 1/8, so every score is exact and ties are plentiful: a bucket whose best score is reached on BOTH
shards must resolve to the smaller global id.  Covered: several segments per shard (global and routed adds), ``buckets``
and ``allow`` in global numbering cut through the segment table, the stored labels (``set_groups`` in global numbering,
``buckets=None``), tombstones, both metrics, buckets no shard has a hit for, the refusals."""
import os
import socket
import sys
from pathlib import Path

import numpy as np
import torch.distributed as dist
import torch.multiprocessing as mp

sys.path.insert(0, str(Path(__file__).resolve().parent))

D_ = 4
N = 260
NB = 9
DEAD = [0, 5, 64, 150, 259]
RADII = {0: (0.25, -0.5, -100.0, 100.0), 1: (1.0, 2.5, 100.0, 0.0)}


def _data():
    rng = np.random.default_rng(43)
    x = (rng.integers(-8, 9, size=(N, D_)) / 8.0).astype(np.float32)
    q = (rng.integers(-8, 9, size=(5, D_)) / 8.0).astype(np.float32)
    q[0] = 1.0                                         # the longest vector of the grid: only a copy of it scores |q|^2 = 4
    x[7] = x[201] = x[120] = q[0]                      # the best score of query 0, on both shards: the tie goes to row 7
    lab = rng.integers(-2, NB + 2, size=N).astype(np.int32)   # -2, -1, NB, NB + 1: unbucketed
    lab[[7, 201, 120]] = 3
    lab[lab == 8] = 2                                  # bucket 8 stays empty everywhere
    allow = rng.random(N) < 0.6
    allow[[7, 201]] = True
    return x, q, lab, allow


def _bytes(res):
    return np.concatenate([np.ascontiguousarray(a).view(np.uint8).reshape(-1) for a in res])


def _ask(ix, out, tag, metric, q, lab, allow, stored):
    for r in RADII[metric]:
        for name, mask in (("all", None), ("mask", allow)):
            out[f"{tag}_{r}_{name}"] = _bytes(ix.facets(q, r, buckets=lab, nbuckets=NB, allow=mask))
            if stored:
                out[f"{tag}_{r}_{name}_stored"] = _bytes(ix.facets(q, r, nbuckets=NB, allow=mask))
    out[f"{tag}_auto_nb"] = _bytes(ix.facets(q[:2], RADII[metric][1], buckets=np.maximum(lab, 0)))   # nbuckets = max + 1
    out[f"{tag}_one"] = _bytes(ix.facets(q[:1], RADII[metric][1], buckets=lab, nbuckets=1))
    out[f"{tag}_nq0"] = _bytes(ix.facets(q[:0], RADII[metric][1], buckets=lab, nbuckets=NB))


def _worker(rank, world, port, out_dir):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from claude_semantic_search_amd.sharded import ShardedFlatIndex, ShardedIndexFacade
        from facets_fakes import FakeFacetIndex
        from related_fakes import merge_lists

        x, q, lab, allow = _data()
        out = {}
        for metric in (0, 1):
            sh = ShardedFlatIndex(D_, metric, index_factory=lambda: FakeFacetIndex(D_, metric), merge=merge_lists(metric))
            sh.add_global(x[:100])
            sh.add_routed(x[100:141])
            sh.add_global(x[141:])
            assert len(sh.segments) >= 2
            sh.set_groups(lab[:130])
            sh.set_groups(lab[130:], row0=130)
            _ask(sh, out, f"sh{metric}", metric, q, lab, allow, True)
            owns = [any(g0 <= r < g0 + m for _, g0, m in sh.segments) for r in (7, 120, 201)]
            np.save(os.path.join(out_dir, f"owns{metric}_{rank}.npy"), np.array(owns))
            sh.mark_deleted(DEAD)
            _ask(sh, out, f"dead{metric}", metric, q, lab, allow, True)
            fac = ShardedIndexFacade(D_, metric, index_factory=lambda: FakeFacetIndex(D_, metric), merge=merge_lists(metric))
            for lo in range(0, N, 37):
                fac.add(x[lo:lo + 37])
            _ask(fac, out, f"fac{metric}", metric, q, lab, allow, False)
            for bad in (dict(buckets=lab[:-1], nbuckets=NB), dict(buckets=None, nbuckets=None), dict(buckets=lab, nbuckets=0),
                        dict(buckets=lab, nbuckets=NB, allow=np.ones(N + 1, bool)), dict(buckets=lab.astype(np.float32))):
                try:
                    fac.facets(q, 0.0, **bad)
                    raise AssertionError(f"facets({list(bad)}) did not raise")
                except ValueError:
                    pass
            try:
                fac.facets(q, float("nan"), buckets=lab, nbuckets=NB)
                raise AssertionError("a NaN threshold did not raise")
            except ValueError:
                pass
        np.savez(os.path.join(out_dir, f"p{rank}.npz"), **out)
    finally:
        dist.destroy_process_group()


def test_sharded_facets_equal_the_unsharded_double(tmp_path):
    from facets_fakes import FakeFacetIndex

    world = 2
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    mp.spawn(_worker, args=(world, port, str(tmp_path)), nprocs=world, join=True)
    got = [np.load(tmp_path / f"p{r}.npz") for r in range(world)]
    x, q, lab, allow = _data()
    live = np.ones(N, bool)
    live[DEAD] = False
    want = {}
    for metric in (0, 1):
        ix = FakeFacetIndex(D_, metric)
        ix.add(x)
        ix.set_groups(lab)
        _ask(ix, want, f"sh{metric}", metric, q, lab, allow, True)
        _ask(ix, want, f"fac{metric}", metric, q, lab, allow, False)

        class Live:   # the unsharded double with the tombstones left out of every mask
            def facets(self, q, r, buckets=None, nbuckets=None, allow=None):
                return ix.facets(q, r, buckets=buckets, nbuckets=nbuckets, allow=live if allow is None else allow & live)

        _ask(Live(), want, f"dead{metric}", metric, q, lab, allow, True)
        # the cases are what they claim
        res = ix.facets(q, RADII[metric][0], buckets=lab, nbuckets=NB)
        assert res.best_id[0, 3] == 7 and res.counts[0, 3] >= 3                 # the tie across the shards: rows 7, 120, 201
        assert res.counts[:, 8].sum() == 0 and (res.best_id[:, 8] == -1).all()
        assert res.unbucketed.sum() > 0 and (res.total == res.counts.sum(1) + res.unbucketed).all()
        everything, nothing = ix.facets(q, RADII[metric][2], buckets=lab, nbuckets=NB), ix.facets(q, RADII[metric][3], buckets=lab, nbuckets=NB)
        assert (everything.total == N).all() and not nothing.total.any()
        dead = Live().facets(q, RADII[metric][2], buckets=lab, nbuckets=NB)
        assert (dead.total == N - len(DEAD)).all()
        owns = np.stack([np.load(tmp_path / f"owns{metric}_{r}.npy") for r in range(world)])
        assert (owns.sum(0) == 1).all() and owns.any(1).all()                    # the tied rows lie on BOTH shards
    for r in range(world):
        assert sorted(got[r].files) == sorted(want)
        for key, val in want.items():
            assert got[r][key].dtype == val.dtype and np.array_equal(got[r][key], val), (key, r)
