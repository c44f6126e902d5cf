"""CPU, world_size 2 over gloo: ``ShardedFlatIndex.where`` / ``set_attribute`` / ``facets(by_attribute=)`` and the facade
against ONE numpy double holding all rows (``where_fakes.FakeWhereIndex``).  Each rank's mask must equal its slice
(``local_rows_of``) of the single index's mask, the count summed over the ranks the single count, and the facets the
same bytes.  Covered: several segments per shard (global and routed adds), ``set_attribute`` calls that cross the shard
boundary and one that touches a single shard only, both types, ``in`` tables, ``allow`` in global numbering,
tombstones, the refusals."""
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
NB = 6
DEAD = [0, 5, 64, 150, 259]
S_I, S_F, S_ONE = 0, 3, 9


def _data():
    rng = np.random.default_rng(47)
    x = (rng.integers(-8, 9, size=(N, D_)) / 8.0).astype(np.float32)
    q = (rng.integers(-8, 9, size=(3, D_)) / 8.0).astype(np.float32)
    code = rng.integers(-1, NB + 2, size=N).astype(np.int32)
    val = rng.standard_normal(N).astype(np.float32)
    val[::17] = np.nan
    allow = rng.random(N) < 0.6
    return x, q, code, val, allow


CALLS = [
    [(S_I, "==", 2)], [(S_I, "in", [0, 3, 5])], [(S_I, "not in", [1])], [(S_F, ">", 0.0), (S_I, ">=", 0)],
    [(S_F, "!=", 0.5), (S_F, "<=", 1.0), (S_I, "!=", 4)], [(S_ONE, "==", 7)], [(S_ONE, "==", -1)], [],
]


def _set(ix, code, val):
    ix.set_attribute(S_I, code[:90])                      # inside the first global add
    ix.set_attribute(S_I, code[90:], row0=90)             # across every later boundary
    ix.set_attribute(S_F, val)
    ix.set_attribute(S_ONE, np.full(10, 7, np.int64), row0=2)   # rows of ONE shard only: the other still has the slot


def _ask(ix, out, tag, q, allow):
    for c, clauses in enumerate(CALLS):
        for name, mask in (("all", None), ("mask", allow)):
            m, cnt = ix.where(clauses, allow=mask, return_count=True)
            out[f"{tag}_{c}_{name}"] = m
            out[f"{tag}_{c}_{name}_n"] = np.array([cnt], np.int64)
            assert np.array_equal(ix.where(clauses, allow=mask), m)
    for name, mask in (("all", None), ("mask", allow)):
        res = ix.facets(q, -100.0, nbuckets=NB, allow=mask, by_attribute=S_I)
        out[f"{tag}_facets_{name}"] = np.concatenate([np.ascontiguousarray(a).view(np.uint8).reshape(-1) for a in res])


def _worker(rank, world, port, out_dir):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from claude_semantic_search_amd.sharded import ShardedFlatIndex, ShardedIndexFacade
        from related_fakes import merge_lists
        from where_fakes import FakeWhereIndex

        x, q, code, val, allow = _data()
        out = {}
        sh = ShardedFlatIndex(D_, 0, index_factory=lambda: FakeWhereIndex(D_, 0), merge=merge_lists(0))
        sh.add_global(x[:100])
        sh.add_routed(x[100:141])
        sh.add_global(x[141:])
        assert len(sh.segments) >= 2
        _set(sh, code, val)
        assert sh.local.attribute_type(S_ONE) == 0 and sh.attribute_type(S_F) == 1 and sh.attribute_type(7) == -1
        _ask(sh, out, "sh", q, allow)
        out["rows"] = sh.local_rows_of(np.arange(N))
        sh.mark_deleted(DEAD)
        _ask(sh, out, "dead", q, allow)
        fac = ShardedIndexFacade(D_, 0, index_factory=lambda: FakeWhereIndex(D_, 0), merge=merge_lists(0))
        for lo in range(0, N, 37):
            fac.add(x[lo:lo + 37])
        _set(fac, code, val)
        _ask(fac, out, "fac", q, allow)
        out["fac_rows"] = fac.sh.local_rows_of(np.arange(N))
        for bad in ([(7, "==", 1)], [(S_F, "in", [1])], [(S_I, "==", 1.5)], [(S_I, "~", 1)]):
            try:
                fac.where(bad)
                raise AssertionError(f"where({bad}) did not raise")
            except ValueError:
                pass
        for bad in (dict(slot=S_I, values=val), dict(slot=S_F, values=code), dict(slot=16, values=code),
                    dict(slot=S_I, values=code, row0=1)):
            try:
                fac.set_attribute(bad.pop("slot"), bad.pop("values"), **bad)
                raise AssertionError("set_attribute did not raise")
            except ValueError:
                pass
        for bad in (dict(by_attribute=S_F, nbuckets=NB), dict(by_attribute=7, nbuckets=NB), dict(by_attribute=S_I),
                    dict(by_attribute=S_I, nbuckets=NB, buckets=code)):
            try:
                fac.facets(q, 0.0, **bad)
                raise AssertionError(f"facets({list(bad)}) did not raise")
            except ValueError:
                pass
        fac.drop_attribute(S_ONE)
        assert fac.attribute_type(S_ONE) == -1
        np.savez(os.path.join(out_dir, f"p{rank}.npz"), **out)
    finally:
        dist.destroy_process_group()


def test_sharded_where_equals_the_slices_of_one_index(tmp_path):
    from where_fakes import FakeWhereIndex

    world = 2
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    mp.spawn(_worker, args=(world, port, str(tmp_path)), nprocs=world, join=True)
    got = [np.load(tmp_path / f"p{r}.npz") for r in range(world)]
    x, q, code, val, allow = _data()
    one = FakeWhereIndex(D_, 0)
    one.add(x)
    _set(one, code, val)
    live = np.ones(N, bool)
    live[DEAD] = False

    class Live:   # the single index with the tombstones left out of every mask
        def where(self, clauses, allow=None, return_count=False):
            return one.where(clauses, allow=live if allow is None else allow & live, return_count=return_count)

        def facets(self, q, r, nbuckets=None, allow=None, by_attribute=None):
            return one.facets(q, r, nbuckets=nbuckets, allow=live if allow is None else allow & live, by_attribute=by_attribute)

    want = {}
    _ask(one, want, "sh", q, allow)
    _ask(one, want, "fac", q, allow)
    _ask(Live(), want, "dead", q, allow)
    for tag, rows_key in (("sh", "rows"), ("dead", "rows"), ("fac", "fac_rows")):
        rows = [got[r][rows_key] for r in range(world)]
        assert sorted(np.concatenate(rows).tolist()) == list(range(N)) and all(r.size for r in rows)
        for c, clauses in enumerate(CALLS):
            for name in ("all", "mask"):
                key = f"{tag}_{c}_{name}"
                for r in range(world):
                    assert got[r][key].dtype == np.bool_ and np.array_equal(got[r][key], want[key][rows[r]]), (key, r)
                    assert int(got[r][key + "_n"][0]) == int(want[key + "_n"][0]), (key, r)       # the SUMMED count
                assert sum(int(got[r][key].sum()) for r in range(world)) == int(want[key + "_n"][0])
        for name in ("all", "mask"):
            key = f"{tag}_facets_{name}"
            for r in range(world):
                assert np.array_equal(got[r][key], want[key]), (key, r)
    # the cases are what they claim: the masks select some rows and leave some out, and S_ONE lies on one shard only
    for c, clauses in enumerate(CALLS[:-1]):
        assert 0 < int(want[f"sh_{c}_all"].sum()) < N, clauses
    held = [np.isin(np.arange(2, 12), got[r]["rows"]).sum() for r in range(world)]
    assert sorted(held) == [0, 10]
