"""GPU: ``HybridStorage.search_recent`` on the HIP index (no test double): 300 chunks at d = 64 with timestamps spread
over a year (every 11th chunk has none, one is deleted), ``now`` passed explicitly.  Against a numpy restatement in fp64
-- inner products (or squared distances) of the rows AS STORED with the query as the index sees it, plus / minus
``weight * 2^(-age / h)`` from the chunks' own timestamps.  The order must equal the fp64 ranking wherever neighbouring
fused values differ by more than 1e-5 (fp32 sums of 64 terms round at ~1e-7; the stored prior and the call's weight
carry one fp32 rounding each, relative 6e-8 of a boost of at most ``weight``); ``similarity`` fields are the RAW ones.
The column is pushed once: a later ``now`` makes no new ``set_priors`` call, a changed half-life makes one."""
from datetime import datetime, timedelta, timezone

import numpy as np
import pytest

from oracle import knn_oracle as ko

pytestmark = pytest.mark.gpu

D_ = 64
N = 300
NOW = datetime(2024, 6, 1, 12, 0, 0, tzinfo=timezone.utc)
DEAD = 17


def _data():
    rng = np.random.default_rng(5)
    q = ko.synth_rows(1, D_, 61)[0]
    raw = ko.synth_rows(N, D_, 62)
    for i in range(0, N, 3):                              # a third of the chunks resemble the query, at falling similarity
        raw[i] = q + (0.5 + 0.01 * i) * raw[i]
    age = rng.random(N) * 365.0                           # days before NOW
    age[::11] = np.nan                                    # no timestamp
    # unit rows and a unit query for both metrics (the L2 storage stores its rows as given): scores of order 1
    return ko.normalize_rows(q[None, :])[0], ko.normalize_rows(raw), age


def _stamp(age, i):
    t = NOW - timedelta(days=float(age))
    return t.replace(tzinfo=None).isoformat() if i % 2 else t.isoformat()      # naive (UTC) and offset spellings


def _storage(tmp_path, raw, age, l2, sharded, record):
    from claude_semantic_search_amd import flat_index as fi
    from claude_semantic_search_amd.chunk import Chunk
    from claude_semantic_search_amd.storage import HybridStorage, StorageConfig

    s = HybridStorage(StorageConfig(data_dir=str(tmp_path / "s"), embedding_dim=D_, auto_save=False, normalize_embeddings=not l2,
                                    sharded=sharded))
    s.initialize()
    inner = s.faiss_index.set_priors

    def recording(priors, row0=0):                        # a thin recorder around the index's own method
        record.append((int(row0), len(priors)))
        return inner(priors, row0=row0)
    s.faiss_index.set_priors = recording
    assert isinstance(s.faiss_index, fi.IndexFlat) != sharded
    chunks = []
    for i in range(N):
        md = {"project_name": "p", "has_code": i % 2 == 0}
        if not np.isnan(age[i]):
            md["timestamp"] = _stamp(age[i], i)
        chunks.append(Chunk(f"c{i}", f"t{i}", md, raw[i]))
    s.add_chunks(chunks)
    assert s.delete_chunk(f"c{DEAD}")
    return s


def _expect(scores, age, later, h, w, l2, top_k, keep=lambda i: True):
    """fp64 ranking of the live chunks: [(chunk number, fused value)] best first, cut at top_k."""
    boost = np.where(np.isnan(age), 0.0, w * np.exp2(-(np.nan_to_num(age) + later) / h))
    fused = scores - boost if l2 else scores + boost
    rows = [i for i in range(N) if i != DEAD and keep(i)]
    rows.sort(key=lambda i: (fused[i] if l2 else -fused[i], i))
    return [(i, fused[i]) for i in rows[:top_k + 1]]


def _check(res, want, scores, what):
    """``want`` carries one rank more than ``res`` may hold, so that the last rank has both neighbours."""
    got = [int(r.chunk_id[1:]) for r in res]
    assert len(got) == len(want) - 1, what
    for pos, (g, (i, f)) in enumerate(zip(got, want)):
        near = [abs(f - want[p][1]) <= 1e-5 for p in (pos - 1, pos + 1) if 0 <= p < len(want)]
        assert g == i or any(near), f"{what}: rank {pos} is c{g}, fp64 says c{i}"
    for r in res:
        i = int(r.chunk_id[1:])
        # the band of tests/test_range_search_gpu.py for rows and queries of at most unit norm: 4 * dpad * 2^-24
        assert abs(r.similarity - scores[i]) <= 4 * 64 * 2.0 ** -24, f"{what}: similarity of c{i} is not the raw one"


@pytest.mark.parametrize("sharded", [False, True], ids=["one_index", "facade"])
@pytest.mark.parametrize("l2", [False, True], ids=["ip", "l2"])
def test_search_recent_ranks_by_similarity_plus_recency(tmp_path, l2, sharded):
    from claude_semantic_search_amd.storage import SearchConfig

    q, raw, age = _data()
    record = []
    s = _storage(tmp_path, raw, age, l2, sharded, record)
    x = s.faiss_index.reconstruct_n(0, N).astype(np.float64)                 # the rows as stored
    if l2:
        scores = ((x - q.astype(np.float64)[None, :]) ** 2).sum(1)
    else:
        scores = x @ ko.normalize_rows(q[None, :])[0].astype(np.float64)
    cfg = SearchConfig(similarity_threshold=-1e30)
    h, w = 30.0, 0.8 if l2 else 0.4                                          # (squared distances of unit rows spread twice as wide)
    plain = [r.chunk_id for r in s.search(q, cfg)]
    assert not record
    res = s.search_recent(q, cfg, half_life_days=h, weight=w, now=NOW)
    want = _expect(scores, age, 0.0, h, w, l2, 10)
    _check(res, want, scores, "first call")
    assert [r.chunk_id for r in res] != plain, "the recency term changed nothing: the case shows nothing"
    assert f"c{DEAD}" not in [r.chunk_id for r in res]
    assert record == [(0, N)]
    # a later now: every chunk ages alike, the column stays, only the weight shrinks
    for later in (10.0, 45.5):
        res = s.search_recent(q, cfg, half_life_days=h, weight=w, now=NOW + timedelta(days=later))
        _check(res, _expect(scores, age, later, h, w, l2, 10), scores, f"{later} days later")
    assert record == [(0, N)], "a later now must not push the column again"
    # a changed half-life pushes it once
    for later in (0.0, 3.0):
        res = s.search_recent(q, cfg, half_life_days=90.0, weight=w, now=NOW + timedelta(days=later))
        _check(res, _expect(scores, age, later, 90.0, w, l2, 10), scores, "half-life 90")
    assert record == [(0, N), (0, N)], "a changed half-life must push the column exactly once"
    # top_k and a filter (not pushed down: max_results rows are fetched and filtered in rank order)
    res = s.search_recent(q, SearchConfig(top_k=4, similarity_threshold=-1e30), filters={"has_code": False},
                          half_life_days=90.0, weight=w, now=NOW)
    _check(res, _expect(scores, age, 0.0, 90.0, w, l2, 4, keep=lambda i: i % 2 == 1), scores, "filter")
    # weight 0 is the plain search
    assert [r.chunk_id for r in s.search_recent(q, cfg, half_life_days=90.0, weight=0.0, now=NOW)] == plain
    s.close()
