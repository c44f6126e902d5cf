"""CPU: the host side of the facet counts -- the argument rules of ``IndexFlat.facets`` (``flat_index.facet_args``), the
``>=`` radius helper at float32 neighbours, the date buckets, the order of the result, and ``HybridStorage.facets`` over
the numpy double ``facets_fakes.FakeFacetIndex`` on a corpus whose counts are known by construction (bucket ids and
their cache, every ``by``, thresholds, tombstones, filters, ``top``, an L2 storage, the stored session labels,
``optimize``, an index without ``facets``).  ``search_range`` hands the index the radius it handed it before the helper
was extracted."""
from datetime import date, timedelta

import numpy as np
import pytest

from claude_semantic_search_amd import flat_index as fi
from claude_semantic_search_amd import storage as st
from claude_semantic_search_amd.storage import Facet, HybridStorage, SearchConfig, SearchResult, StorageConfig
from facets_fakes import D_, LEVELS, N, Q, FakeFacetIndex, as_tuples, bucket_value, corpus, expected
from related_fakes import FakeIndex

BYS = ("project_name", "session_id", "chunk_type", "has_code", "has_tools", "day", "week", "month")


# ------------------------------------------------------------------------------------------------ IndexFlat.facets arguments
def test_facet_args():
    lab = np.array([0, 3, -1, 2], np.int64)
    t, b, nb = fi.facet_args(0.5, lab, None, 4)
    assert t == 0.5 and b.dtype == np.int32 and b.tolist() == [0, 3, -1, 2] and nb == 4          # max + 1
    assert fi.facet_args(0.5, np.full(4, -7), None, 4)[2] == 1                                  # ... at least 1
    assert fi.facet_args(0.5, np.zeros(0, np.int32), None, 0)[2] == 1
    assert fi.facet_args(float("-inf"), None, np.int64(9), 4)[1:] == (None, 9)
    assert fi.facet_args(1, lab, fi.MAX_FACET_BUCKETS, 4)[2] == fi.MAX_FACET_BUCKETS == 1 << 20
    for bad in (dict(thresh=float("nan")), dict(buckets=None, nbuckets=None), dict(nbuckets=0), dict(nbuckets=-1),
                dict(nbuckets=fi.MAX_FACET_BUCKETS + 1), dict(nbuckets=2.0), dict(nbuckets=True), dict(buckets=lab[:3]),
                dict(buckets=lab.astype(np.float32)), dict(buckets=lab > 0), dict(buckets=lab.reshape(2, 2)),
                dict(buckets=lab + 2 ** 31), dict(buckets=["a", "b", "c", "d"])):
        args = dict(thresh=0.5, buckets=lab, nbuckets=4)
        args.update(bad)
        with pytest.raises(ValueError, match="facets"):
            fi.facet_args(args["thresh"], args["buckets"], args["nbuckets"], 4)
    with pytest.raises((ValueError, TypeError)):
        fi.facet_args("x", lab, 4, 4)


# ------------------------------------------------------------------------------------------------ the radius helper
def _f32_around(v, steps=3):
    out = [np.float32(v)]
    for _ in range(steps):
        out.insert(0, np.nextafter(out[0], np.float32(-np.inf)))
        out.append(np.nextafter(out[-1], np.float32(np.inf)))
    return out


@pytest.mark.parametrize("base", [0.0, 0.1, 0.7, 1.0, -0.25, 2.0, 1e-30, 3e38])
def test_strict_radius_means_greater_or_equal_at_float32_neighbours(base):
    f = _f32_around(base)
    between = [(float(a) + float(b)) / 2 for a, b in zip(f, f[1:])]          # doubles that are no float32
    for thr in [float(v) for v in f] + between:
        r_ip, r_l2 = st.strict_radius(thr, True), st.strict_radius(thr, False)
        assert r_ip.dtype == np.float32 and r_l2.dtype == np.float32
        for s in _f32_around(base, 6):
            assert (s > r_ip) == (float(s) >= thr), (thr, float(s))
            assert (s < r_l2) == (float(s) <= thr), (thr, float(s))


def _radius_before_extraction(thr, similarity):
    """``search_range``'s own lines before ``strict_radius`` was extracted from it (the overflow warning silenced)."""
    with np.errstate(over="ignore"):
        t32 = np.float32(thr)
        if similarity:
            if float(t32) < thr:
                t32 = np.nextafter(t32, np.float32(np.inf))
            return np.nextafter(t32, np.float32(-np.inf))
        if float(t32) > thr:
            t32 = np.nextafter(t32, np.float32(-np.inf))
        return np.nextafter(t32, np.float32(np.inf))


# ------------------------------------------------------------------------------------------------ dates and order
def test_date_buckets_against_the_calendar():
    for day in list(range(-800, 800, 37)) + list(range(19700, 20100)):
        d = date(1970, 1, 1) + timedelta(days=day)
        for frac in (0.0, 0.5, 0.999):
            assert st.facet_date_value(st.facet_date_key(day + frac, "day"), "day") == d.isoformat()
            assert st.facet_date_value(st.facet_date_key(day + frac, "week"), "week") == (d - timedelta(days=d.weekday())).isoformat()
            assert st.facet_date_value(st.facet_date_key(day + frac, "month"), "month") == d.replace(day=1).isoformat()
    assert st.facet_date_key(float("nan"), "day") is None
    assert st.facet_date_key(st.timestamp_days("2024-03-31T23:59:59Z"), "month") == 2024 * 12 + 2


def test_order_and_top():
    f = lambda v, c, s: Facet(v, c, SearchResult(f"id{v}", s))
    rows = [f("d", 2, 0.5), f("a", 2, 0.9), f("c", 7, 0.1), f("b", 2, 0.9), f("e", 1, 0.99)]
    assert [x.value for x in st.order_facets(rows, True)] == ["c", "a", "b", "d", "e"]          # count, best, value
    assert [x.value for x in st.order_facets(rows, False)] == ["c", "d", "a", "b", "e"]         # distances: smaller first
    assert [x.value for x in st.order_facets(rows, True, top=2)] == ["c", "a"]
    assert st.order_facets(rows, True, top=0) == [] and len(st.order_facets(rows, True, top=99)) == 5


# ------------------------------------------------------------------------------------------------ HybridStorage.facets
def _use(monkeypatch, cls):
    monkeypatch.setattr(fi, "IndexFlat", cls)
    monkeypatch.setattr(fi, "IndexFlatIP", lambda d, device=0: cls(d, 0, device))
    monkeypatch.setattr(fi, "IndexFlatL2", lambda d, device=0: cls(d, 1, device))


def _storage(tmp_path, pushdown=False, l2=False, n=N):
    s = HybridStorage(StorageConfig(data_dir=str(tmp_path / "s"), embedding_dim=D_, normalize_embeddings=not l2,
                                    auto_save=False, filter_pushdown=pushdown))
    s.initialize()
    if n:
        s.add_chunks(corpus(0, n))
    return s


@pytest.mark.parametrize("by", BYS)
def test_every_by_at_several_thresholds(tmp_path, monkeypatch, by):
    _use(monkeypatch, FakeFacetIndex)
    s = _storage(tmp_path)
    for thr in (0.4, 0.0, -1.0, 0.95):
        got = as_tuples(s.facets(Q, by=by, threshold=thr))
        assert got == expected(by, thr), (by, thr)
    total, missing, rows = as_tuples(s.facets(Q, by=by, threshold=0.4))
    assert total == N // 2 and total == missing + sum(r[1] for r in rows)
    assert (missing > 0) == (by in ("project_name", "session_id", "day", "week", "month"))
    assert as_tuples(s.facets(Q, by=by, threshold=0.95)) == (0, 0, [])
    # the default threshold is the config's, and the best hit is a SearchResult under the config
    cfg = SearchConfig(similarity_threshold=0.6, include_text=False)
    res = s.facets(Q, by=by, config=cfg)
    assert as_tuples(res) == expected(by, 0.6)
    assert all(f.best.text is None and f.best.metadata is not None and f.best.chunk is None for f in res.buckets)
    assert all(abs(f.best.similarity - LEVELS[int(f.best.chunk_id[1:]) % 6]) < 1e-6 for f in res.buckets)
    s.close()


def test_bucket_ids_are_dense_and_cached_under_the_stamp_of_the_allow_mask(tmp_path, monkeypatch):
    _use(monkeypatch, FakeFacetIndex)
    s = _storage(tmp_path, n=60)
    ids, values = s._facet_buckets("project_name", 60)
    assert ids.dtype == np.int32 and ids.shape == (60,) and values == ["alpha", "beta", "gamma"]     # first appearance
    assert [(-1 if bucket_value(i, "project_name") is None else values.index(bucket_value(i, "project_name")))
            for i in range(60)] == ids.tolist()
    again = s._facet_buckets("project_name", 60)
    assert again[0] is ids and again[1] is values                                # cached: the same objects
    hc, hv = s._facet_buckets("has_code", 60)
    assert hv == [True, False] and hc.tolist() == [i % 2 for i in range(60)]
    mi, mv = s._facet_buckets("month", 60)
    assert mv == sorted(mv) and mv[0] == "2024-01-01" and (mi == -1).sum() == 6  # every tenth chunk has no timestamp
    assert s._facet_buckets("project_name", 60)[0] is ids                        # one entry per `by`
    s.add_chunks(corpus(60, 90))                                                 # the stamp moves: rebuilt
    ids2, _ = s._facet_buckets("project_name", 90)
    assert ids2 is not ids and ids2.shape == (90,) and ids2[:60].tolist() == ids.tolist()
    assert s.delete_chunk("c0")
    ids3, _ = s._facet_buckets("project_name", 90)
    assert ids3[0] == -1 and ids3[1:].tolist() == ids2[1:].tolist()               # a row without a chunk: -1
    s.close()


def test_too_many_distinct_values_raise(tmp_path, monkeypatch):
    _use(monkeypatch, FakeFacetIndex)
    monkeypatch.setattr(fi, "MAX_FACET_BUCKETS", 2)
    s = _storage(tmp_path, n=60)
    with pytest.raises(ValueError, match="3 distinct values"):
        s.facets(Q, by="project_name", threshold=0.0)
    assert s.facets(Q, by="has_code", threshold=0.0).total == 50
    s.close()


def test_threshold_is_inclusive_at_exactly_a_chunks_similarity(tmp_path, monkeypatch):
    _use(monkeypatch, FakeFacetIndex)
    s = _storage(tmp_path)
    at = float(np.float32(0.7))                                                  # the double's score of the 0.7 chunks
    assert s.facets(Q, by="has_code", threshold=at).total == N // 3
    assert s.facets(Q, by="has_code", threshold=float(np.nextafter(np.float32(0.7), np.float32(1)))).total == N // 6
    s.close()


@pytest.mark.parametrize("pushdown", [False, True])
def test_tombstones_filters_and_top(tmp_path, monkeypatch, pushdown):
    _use(monkeypatch, FakeFacetIndex)
    s = _storage(tmp_path, pushdown)
    dead = {0, 6, 7, 100, 239}
    for i in dead:
        assert s.delete_chunk(f"c{i}")
    for by in BYS:
        assert as_tuples(s.facets(Q, by=by, threshold=0.2)) == expected(by, 0.2, dead=dead), by
    # filters always go into the mask, whatever filter_pushdown says: a count cannot be filtered afterwards
    got = s.facets(Q, by="project_name", threshold=0.2, filters={"has_code": True})
    assert as_tuples(got) == expected("project_name", 0.2, dead=dead, keep=lambda i: i % 2 == 0)
    assert s.faiss_index.calls[-1] == ("facets", False, 3, True)
    got = s.facets(Q, by="month", threshold=0.2, filters={"chunk_type": ["code", "tool"], "project_name": "ALPH"})
    assert as_tuples(got) == expected("month", 0.2, dead=dead, keep=lambda i: i % 3 != 0 and (i // 6) % 4 == 0)
    for top in (1, 3, 100):
        assert as_tuples(s.facets(Q, by="week", threshold=0.2, top=top)) == expected("week", 0.2, dead=dead, top=top)
    full = s.facets(Q, by="week", threshold=0.2)
    cut = s.facets(Q, by="week", threshold=0.2, top=0)
    assert cut.buckets == [] and (cut.total, cut.missing) == (full.total, full.missing)
    s.close()


def test_session_facet_counts_over_the_stored_labels_and_uploads_nothing(tmp_path, monkeypatch):
    _use(monkeypatch, FakeFacetIndex)
    s = _storage(tmp_path)
    assert as_tuples(s.facets(Q, by="session_id", threshold=0.2)) == expected("session_id", 0.2)
    assert s.faiss_index.calls[-1] == ("facets", True, 8, False)                  # buckets=None reached the index
    assert [c for c in s.faiss_index.calls if c[0] == "set_groups"] == [("set_groups", 0, N)]
    s.facets(Q, by="project_name", threshold=0.2)
    assert s.faiss_index.calls[-1] == ("facets", False, 3, False)                 # every other `by` hands a column over
    # consistent after a compaction: rows renumbered, labels pushed again, bucket ids rebuilt
    dead = {1, 2, 3, 60, 61}
    for i in dead:
        assert s.delete_chunk(f"c{i}")
    before = {by: as_tuples(s.facets(Q, by=by, threshold=0.2)) for by in BYS}
    s.optimize()
    assert s.faiss_index.ntotal == N - len(dead)
    for by in BYS:
        assert as_tuples(s.facets(Q, by=by, threshold=0.2)) == before[by] == expected(by, 0.2, dead=dead), by
    s.close()


def test_l2_storage_counts_distances_up_to_the_threshold(tmp_path, monkeypatch):
    _use(monkeypatch, FakeFacetIndex)
    s = _storage(tmp_path, l2=True)
    for by in ("project_name", "month", "session_id"):
        for thr in (0.7, 1.0, 5.0, 0.1):                                          # 2 - 2 cos: 0.2, 0.6, 1.0, 1.4, 1.8, 2.4
            assert as_tuples(s.facets(Q, by=by, threshold=thr)) == expected(by, thr, l2=True), (by, thr)
    res = s.facets(Q, by="has_code", threshold=0.7)
    assert res.total == N // 3
    assert [round(f.best.similarity, 5) for f in res.buckets] == [0.2, 0.6]       # squared distances, even chunks first
    s.close()


def test_refusals_and_empty_storage(tmp_path, monkeypatch):
    _use(monkeypatch, FakeFacetIndex)
    s = _storage(tmp_path, n=0)
    assert as_tuples(s.facets(Q)) == (0, 0, [])
    s.add_chunks(corpus(0, 12))
    for bad in ("file_path", "", "Project_name", None, "year"):
        with pytest.raises(ValueError, match="by="):
            s.facets(Q, by=bad)
    with pytest.raises(ValueError, match="NaN"):
        s.facets(Q, threshold=float("nan"))
    assert s.facets(Q).total == 10                                               # the config's threshold 0.0: all but -0.2
    s.close()


def test_an_index_without_facets_raises(tmp_path, monkeypatch):
    _use(monkeypatch, FakeIndex)
    s = _storage(tmp_path, n=12)
    with pytest.raises(NotImplementedError, match="facets"):
        s.facets(Q)
    assert len(s.search(Q)) == 10
    s.close()


@pytest.mark.parametrize("l2", [False, True])
def test_search_range_hands_over_the_radius_it_always_did(tmp_path, monkeypatch, l2):
    _use(monkeypatch, FakeFacetIndex)
    s = _storage(tmp_path, l2=l2)
    f = _f32_around(0.7, 2)
    for thr in [0.4, 0.0, 1.4, -3.0, 1e40, float(f[0])] + [(float(a) + float(b)) / 2 for a, b in zip(f, f[1:])]:
        res = s.search_range(Q, threshold=thr)
        call = s.faiss_index.calls[-1]
        want = _radius_before_extraction(thr, not l2)
        assert call[0] == "range_search" and call[1].view(np.uint32) == np.float32(want).view(np.uint32), thr
        # (inner product against the unit axis: the double's score IS float32(level); distances stay clear of 0.7)
        score = (lambda i: 2.0 - 2.0 * LEVELS[i % 6]) if l2 else (lambda i: float(np.float32(LEVELS[i % 6])))
        keep = [i for i in range(N) if (score(i) <= thr + 1e-5 if l2 else score(i) >= thr)]
        keep.sort(key=lambda i: (score(i) if l2 else -score(i), i))
        assert [r.chunk_id for r in res] == [f"c{i}" for i in keep], thr
    s.close()
