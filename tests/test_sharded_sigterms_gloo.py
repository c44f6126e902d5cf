"""CPU, world_size 2 and 3 over gloo: ``ShardedFlatIndex.subset_terms`` / ``significant_terms`` and the facade equal the
unsharded numpy double (``sigterms_fakes.FakeSigIndex``) byte for byte -- terms, both counts, the score's 8 bytes and the
set sizes.  The counts are integers that add up over the shards, and both sides rank with
``lexical.significant_from_counts``.  Covered: several segments per shard, rows without lists, an EMPTY shard (three
ranks, two routed adds), a shard whose part of the selection is empty, a background mask, tombstones, the refusals."""
import os
import socket
import sys
from pathlib import Path

import numpy as np
import pytest
import torch.distributed as dist
import torch.multiprocessing as mp

sys.path.insert(0, str(Path(__file__).resolve().parent))

D_ = 4
N = 230
T = 200            # rows 200.. have no list
V = 60
PLANT = (7, 8, 9)
CALLS = ((20, 2), (1, 1), (256, 1), (5, 50))
DEAD = [1, 64, 150, 199, 229]


def _data():
    rng = np.random.default_rng(41)
    x = (rng.integers(-8, 9, size=(N, D_)) / 8.0).astype(np.float32)
    lists = [np.floor(V * rng.random(int(rng.integers(0, 25))) ** 2).astype(np.int64) for _ in range(T)]
    for r in range(60, 90):
        lists[r] = np.concatenate([lists[r], np.array(PLANT) + 1000])     # three terms of one stretch of rows
    sel = rng.random(N) < 0.3
    sel[60:90] = True
    low = np.arange(N) < 40                                                # lives on the first shard alone
    back = sel | (rng.random(N) < 0.5)
    return x, lists, {"rand": sel, "low": low, "none": np.zeros(N, bool), "tail": np.arange(N) >= T}, back


def _bytes(res):
    """Every field of a result as raw bytes in one uint8 array."""
    return np.concatenate([np.ascontiguousarray(a).view(np.uint8) for a in
                           (res.terms, res.fg, res.bg, res.score, np.array([res.n_fg, res.n_bg], np.int64))])


def _ask(ix, out, tag, sels, back):
    for name, sel in list(sels.items()) + [("all", None)]:
        t, f = ix.subset_terms(sel)
        out[f"{tag}_sub_{name}"] = np.concatenate([t.astype(np.int64), f])
        for m, mc in CALLS:
            out[f"{tag}_sig_{name}_{m}_{mc}"] = _bytes(ix.significant_terms(allow=sel, m=m, min_count=mc))
        if sel is not None:
            out[f"{tag}_bg_{name}"] = _bytes(ix.significant_terms(allow=sel & back, m=20, min_count=1, background=back))
    out[f"{tag}_bg_all"] = _bytes(ix.significant_terms(allow=back & sels["rand"], m=256, min_count=1, background=back))


def _build(sh, x, lists, world):
    if world == 3:                                       # two routed adds: the third shard stays EMPTY
        sh.add_routed(x[:120])
        sh.add_routed(x[120:])
        assert sh.shard_sizes[2] == 0
    else:
        sh.add_global(x[:100])
        sh.add_routed(x[100:141])
        sh.add_global(x[141:])
        assert len(sh.segments) >= 2
    sh.set_terms(lists[:70])
    sh.set_terms(lists[70:])


def _worker(rank, world, port, out_dir):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from claude_semantic_search_amd.sharded import ShardedFlatIndex, ShardedIndexFacade
        from related_fakes import merge_lists
        from sigterms_fakes import FakeSigIndex

        x, lists, sels, back = _data()
        out = {}
        sh = ShardedFlatIndex(D_, 0, index_factory=lambda: FakeSigIndex(D_, 0), merge=merge_lists(0))
        out["nolists"] = _bytes(sh.significant_terms())                   # an index without rows or lists
        _build(sh, x, lists, world)
        _ask(sh, out, "sh", sels, back)
        sh.mark_deleted(DEAD)
        _ask(sh, out, "dead", sels, back)
        fac = ShardedIndexFacade(D_, 0, index_factory=lambda: FakeSigIndex(D_, 0), merge=merge_lists(0))
        for lo in range(0, N, 37):
            fac.add(x[lo:lo + 37])
        fac.set_terms(lists)
        _ask(fac, out, "fac", sels, back)
        for bad in (dict(m=0), dict(m=257), dict(min_count=0), dict(allow=np.ones(N - 1, bool)),
                    dict(background=np.ones(N + 1, bool)), dict(allow=sels["rand"], background=~sels["rand"])):
            try:
                fac.significant_terms(**bad)
                raise AssertionError(f"significant_terms({list(bad)}) did not raise")
            except ValueError:
                pass
        np.savez(os.path.join(out_dir, f"p{rank}.npz"), **out)
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_sharded_significant_terms_equal_the_unsharded_double(tmp_path, world):
    from sigterms_fakes import FakeSigIndex

    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    mp.spawn(_worker, args=(world, port, str(tmp_path)), nprocs=world, join=True)
    got = [np.load(tmp_path / f"p{r}.npz") for r in range(world)]
    x, lists, sels, back = _data()
    ix = FakeSigIndex(D_, 0)
    want = {"nolists": _bytes(ix.significant_terms())}
    ix.add(x)
    ix.set_terms(lists)
    _ask(ix, want, "sh", sels, back)
    _ask(ix, want, "fac", sels, back)
    # tombstones leave the selection and a background MASK; without a mask the background stays every row with a list
    live = np.ones(N, bool)
    live[DEAD] = False
    for name, sel in list(sels.items()) + [("all", None)]:
        cut = live if sel is None else sel & live
        t, f = ix.subset_terms(cut)
        want[f"dead_sub_{name}"] = np.concatenate([t.astype(np.int64), f])
        for m, mc in CALLS:
            want[f"dead_sig_{name}_{m}_{mc}"] = _bytes(ix.significant_terms(allow=cut, m=m, min_count=mc))
        if sel is not None:
            want[f"dead_bg_{name}"] = _bytes(ix.significant_terms(allow=sel & back & live, m=20, min_count=1, background=back & live))
    want["dead_bg_all"] = _bytes(ix.significant_terms(allow=back & sels["rand"] & live, m=256, min_count=1, background=back & live))
    for r in range(world):
        assert sorted(got[r].files) == sorted(want)
        for key, val in want.items():
            assert got[r][key].dtype == val.dtype and np.array_equal(got[r][key], val), (key, r)
    # the cases are what they claim: the planted terms lead, a mask changes the answer, some answers are short or empty
    first = ix.significant_terms(allow=sels["rand"], m=3, min_count=2)
    assert sorted(first.terms.tolist()) == [p + 1000 for p in PLANT]
    assert not np.array_equal(want["sh_sig_rand_20_2"], want["sh_bg_rand"])
    assert ix.significant_terms(allow=sels["none"]).terms.size == 0 and ix.significant_terms(allow=sels["tail"]).terms.size == 0
    assert 0 < ix.significant_terms(allow=sels["rand"], m=256, min_count=1).terms.size < 256
    assert ix.significant_terms(allow=sels["low"], m=20, min_count=1).terms.size > 0
