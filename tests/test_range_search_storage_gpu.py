"""GPU: ``HybridStorage.search_range`` on the HIP index (no test double) and ``ShardedFlatIndex.range_search`` as two
ranks on one GPU (gloo moving the lists, as ``tests/test_sharded_gpu.py`` rehearses the top-k path).

Truth is fp64 numpy on the fp32 rows as stored (``oracle.normalize_rows``), with the band of
``tests/test_range_search_gpu.py``: ``dpad * 2^-24 * ||x|| * ||q||`` for inner products, ``4 * dpad * 2^-24 *
max(||x||^2, ||q||^2)`` for squared distances (derivation there).  Chunks whose fp64 score is clearly on one side of the
threshold must be in / out; every reported similarity lies within the band of its fp64 value and satisfies the
threshold itself."""
import os
import socket

import numpy as np
import pytest

from oracle import knn_oracle as ko

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
N, D_ = 6000, 64


def _storage(tmp_path, name, x, l2=False, pushdown=False):
    from claude_semantic_search_amd.chunk import Chunk
    from claude_semantic_search_amd.storage import HybridStorage, StorageConfig

    s = HybridStorage(StorageConfig(data_dir=str(tmp_path / name), embedding_dim=D_, normalize_embeddings=not l2,
                                    auto_save=False, filter_pushdown=pushdown))
    s.initialize()
    s.add_chunks([Chunk(f"c{i}", f"t{i}", {"session_id": f"s{i % 4}", "project_name": "p"}, x[i]) for i in range(x.shape[0])])
    return s


def _check(res, S, band, thr, l2, live, what):
    """res: List[SearchResult]; S / band: fp64 score and band per row; live: rows that may be returned."""
    ids = np.array([int(r.chunk_id[1:]) for r in res], dtype=np.int64)
    sims = np.array([r.similarity for r in res], dtype=np.float64)
    assert len(set(ids.tolist())) == ids.shape[0], what
    got = np.zeros(S.shape[0], bool)
    got[ids] = True
    if l2:
        sure, maybe = S < thr - band, S <= thr + band
        assert (sims <= thr).all() and (np.diff(sims) >= 0).all(), what
    else:
        sure, maybe = S > thr + band, S >= thr - band
        assert (sims >= thr).all() and (np.diff(sims) <= 0).all(), what
    assert not (sure & live & ~got).any(), f"{what}: chunks clearly inside the threshold are missing"
    assert not (got & ~(maybe & live)).any(), f"{what}: chunks clearly outside (or dead / filtered) returned"
    assert (np.abs(sims - S[ids]) <= band[ids]).all(), what
    hits, in_band = int((sure & live).sum()), int((maybe & ~sure & live).sum())
    assert in_band <= (5 if hits < 100 else 0.05 * hits), f"{what}: {in_band} rows inside the band, {hits} clear hits"
    return ids


@pytest.mark.parametrize("pushdown", [False, True])
def test_more_hits_than_search_can_give_filters_tombstones_and_limit(tmp_path, pushdown):
    from claude_semantic_search_amd import flat_index as fi
    from claude_semantic_search_amd.storage import SearchConfig

    raw = ko.synth_rows(N, D_, 41)
    x = ko.normalize_rows(raw)                              # what the index stores
    q = ko.synth_rows(1, D_, 42)[0]
    qn = ko.normalize_rows(q)[0].astype(np.float64)
    S = x.astype(np.float64) @ qn
    band = D_ * U * np.sqrt((x.astype(np.float64) ** 2).sum(1)) * np.sqrt((qn ** 2).sum())
    s = _storage(tmp_path, "ip", raw, pushdown=pushdown)
    assert type(s.faiss_index) is fi.IndexFlatIP and s.faiss_index._h is not None
    live = np.ones(N, bool)
    res = s.search_range(q, threshold=0.0)
    ids = _check(res, S, band, 0.0, False, live, "all chunks at least 0.0 similar")
    assert ids.shape[0] > fi.MAX_K                          # more than search() can ever return
    assert len(s.search(q, SearchConfig(top_k=10 ** 6, max_results=10 ** 6))) == fi.MAX_K
    assert res[0].text == f"t{ids[0]}" and res[0].chunk.id == res[0].chunk_id
    # limit: the best `limit` of the same list
    assert [r.chunk_id for r in s.search_range(q, threshold=0.0, limit=7)] == [r.chunk_id for r in res[:7]]
    # the threshold defaults to the config's
    cfg = SearchConfig(similarity_threshold=0.25, top_k=3, max_results=5)
    res25 = s.search_range(q, config=cfg)
    _check(res25, S, band, 0.25, False, live, "threshold from the config")
    assert len(res25) > 5
    # tombstones: the best hit and every fifth chunk leave SQLite, their rows stay in the index
    dead = [int(ids[0])] + list(range(0, N, 5))
    for i in set(dead):
        assert s.delete_chunk(f"c{i}")
    live[dead] = False
    assert s.faiss_index.ntotal == N
    _check(s.search_range(q, threshold=0.0), S, band, 0.0, False, live, "tombstones")
    # filters
    f_live = live & (np.arange(N) % 4 == 1)
    fres = s.search_range(q, threshold=0.0, filters={"session_id": "s1"})
    _check(fres, S, band, 0.0, False, f_live, "filter")
    assert len(fres) > 100
    s.close()


def test_pushdown_on_and_off_give_the_same_list(tmp_path):
    raw = ko.synth_rows(N, D_, 43)
    q = ko.synth_rows(1, D_, 44)[0]
    lists = []
    for pushdown in (False, True):
        s = _storage(tmp_path, f"pd{int(pushdown)}", raw, pushdown=pushdown)
        for i in range(0, N, 3):
            assert s.delete_chunk(f"c{i}")
        lists.append([[(r.chunk_id, r.similarity) for r in s.search_range(q, threshold=t, filters=f, limit=lim)]
                      for t, f, lim in ((0.0, None, None), (0.1, {"session_id": ["s1", "s2"]}, None), (-1.0, {"session_id": "s3"}, 50))])
        s.close()
    assert lists[0] == lists[1]
    assert len(lists[0][0]) > 1500 and len(lists[0][1]) > 100 and len(lists[0][2]) == 50


def test_l2_storage_means_distance_at_most_threshold(tmp_path):
    raw = ko.synth_rows(N, D_, 45)                          # stored as given (no normalisation): norms around 8
    q = ko.synth_rows(1, D_, 46)[0]
    x64, q64 = raw.astype(np.float64), q.astype(np.float64)
    S = ((x64 - q64[None, :]) ** 2).sum(1)
    band = 4 * D_ * U * np.maximum((x64 ** 2).sum(1), (q64 ** 2).sum())
    thr = float(np.median(S))
    s = _storage(tmp_path, "l2", raw, l2=True)
    res = s.search_range(q, threshold=thr)
    ids = _check(res, S, band, thr, True, np.ones(N, bool), "L2 storage")
    assert abs(ids.shape[0] - N // 2) <= 3
    assert s.search_range(q, threshold=-1.0) == []
    s.close()


# ------------------------------------------------------------------ two ranks on one GPU
def _rank(rank, world, port, out_dir):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import torch
    import torch.distributed as dist

    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from claude_semantic_search_amd.sharded import ShardedFlatIndex

        torch.cuda.set_device(0)
        d = 768
        out = {}
        for metric, radius in ((0, 0.08), (1, 1.84)):
            sh = ShardedFlatIndex(d, metric, device_index=0)
            sh.add_global(ko.normalize_rows(ko.synth_rows(100_000, d, 4)))      # (host rows: the same bits as the unsharded index)
            sh.add_routed(ko.normalize_rows(ko.synth_rows(500, d, 8)))        # second segment on rank 0
            sh.add_global(ko.normalize_rows(ko.synth_rows(1000, d, 9)))
            q = ko.normalize_rows(ko.synth_rows(20, d, 5))
            n = sh.ntotal_global
            allow = (np.arange(n) % 3) != 1
            out[f"m{metric}"] = sh.range_search(q, radius)
            sh.mark_deleted([5, 100_100, n - 1])
            out[f"m{metric}masked"] = sh.range_search(q, radius, allow=allow)
            out[f"m{metric}none"] = sh.range_search(q, 2.0 if metric == 0 else 0.0)
            sh.local.close()
        np.savez(os.path.join(out_dir, f"g{rank}.npz"), **{f"{k}_{n}": v for k, t in out.items() for n, v in zip("LDI", t)})
    finally:
        dist.destroy_process_group()


def test_two_ranks_on_one_gpu_equal_one_unsharded_index(tmp_path):
    """The unsharded index gives the same bits (the sweep's arithmetic per row does not depend on where the row lives);
    the unsharded result itself is checked against fp64 by ``tests/test_range_search_gpu.py``'s rule."""
    import torch.multiprocessing as mp

    from claude_semantic_search_amd.flat_index import IndexFlat
    from test_range_search_gpu import _assert_cap, _check, _truth

    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    mp.spawn(_rank, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    d = 768
    x = ko.normalize_rows(np.concatenate([ko.synth_rows(100_000, d, 4), ko.synth_rows(500, d, 8), ko.synth_rows(1000, d, 9)]))
    q = ko.normalize_rows(ko.synth_rows(20, d, 5))
    n = x.shape[0]
    allow = (np.arange(n) % 3) != 1
    allow[[5, 100_100, n - 1]] = False
    got = [np.load(tmp_path / f"g{r}.npz") for r in range(2)]
    for metric, radius in ((0, 0.08), (1, 1.84)):
        whole = IndexFlat(d, metric)
        whole.add(x)
        S, band = _truth(x, q, metric)
        for key, want, ok in ((f"m{metric}", whole.range_search(q, radius), None),
                              (f"m{metric}masked", whole.range_search(q, radius, allow=allow), allow)):
            hits, in_band = _check(want, S, band, radius, metric, key, allowed=ok)
            _assert_cap(hits, in_band, key)
            assert hits > 1000
            for r in range(2):
                for nm, w in zip("LDI", want):
                    g = got[r][f"{key}_{nm}"]
                    assert g.dtype == w.dtype and np.array_equal(g, w), f"rank {r} {key}: {nm} differs from one index"
        for r in range(2):
            assert got[r][f"m{metric}none_L"].tolist() == [0] * 21 and got[r][f"m{metric}none_D"].shape == (0,)
        whole.close()
