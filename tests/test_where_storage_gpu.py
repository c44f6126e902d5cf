"""GPU: ``HybridStorage`` with ``StorageConfig.attribute_filters`` on and off over the corpus of ``facets_fakes`` (imported,
not edited; every chunk is given a ``word_count`` here).  The binding rule: with the option on every method returns what it
returns with it off under the same ``filter_pushdown`` -- ids, order and similarities -- because only the place where
the allow mask is computed changes (``IndexFlat.where`` over synced attribute columns against the host loop
``_allow_mask``).  Every tenth chunk of the corpus has no timestamp, and the host comparison of ``None`` with a bound
raises ``TypeError``: a timestamp range therefore raises in BOTH storages there (``compile_filters`` declines, the
fallback raises), and is compared for results on a second pair of storages built from the chunks that have one."""
import copy

import numpy as np
import pytest

from claude_semantic_search_amd.chunk import Chunk
from claude_semantic_search_amd.storage import HybridStorage, SearchConfig, StorageConfig
from facets_fakes import D_, N, Q, T0, corpus, fields

pytestmark = pytest.mark.gpu

CFG = SearchConfig(top_k=12, similarity_threshold=-1.0, max_results=50)
STAMP = lambda i: fields(i)["timestamp"]   # noqa: E731

FILTERS = {
    "exact": {"chunk_type": "code"},
    "exact flag": {"has_code": True},
    "exact session": {"session_id": "s20"},
    "list": {"chunk_type": ["code", "tool"], "project_name": ["alpha", "gamma", "nobody"]},
    "substring in the wrong case": {"project_name": "ALPH"},
    "word_count range": {"word_count": {"gte": 60, "lt": 400}},
    "combined": {"project_name": "eta", "has_tools": False, "word_count": {"gt": 30}, "chunk_type": ["conversation", "tool"]},
    "not a column": {"no_such_key": "x", "related_to": "c3", "has_code": False},
    "nothing passes": {"chunk_type": "none of them"},
    "empty": {},
}
TS_FILTERS = {
    "timestamp range": {"timestamp": {"gte": STAMP(20), "lt": STAMP(151)}},
    "timestamp range, a bound between stored values": {"timestamp": {"gt": "2024-03", "lte": "2024-09-15T00:00:00Zzz"}},
    "timestamp and more": {"timestamp": {"gte": STAMP(40)}, "has_code": True, "project_name": "a"},
    "timestamp exact": {"timestamp": STAMP(21)},
}
UNCOMPILABLE = {"word_count": {"gte": 2.5}}       # a bound that is not an integer: compile_filters declines


def _chunks(lo, hi, keep=lambda i: True, **extra):
    out = []
    for i, c in zip(range(lo, hi), corpus(lo, hi)):
        if keep(i):
            out.append(Chunk(c.id, c.text, {**c.metadata, "word_count": 3 * i, **extra}, c.embedding))
    return out


def _pair(tmp_path, chunks):
    pair = []
    for name, on in (("on", True), ("off", False)):
        s = HybridStorage(StorageConfig(data_dir=str(tmp_path / name), embedding_dim=D_, auto_save=False, filter_pushdown=True,
                                        attribute_filters=on))
        s.initialize()
        s.add_chunks(copy.deepcopy(chunks))
        pair.append(s)
    return pair


def _hits(res):
    return [(r.chunk_id, np.float32(r.similarity).tobytes()) for r in res]


def _answers(s, f):
    return {"search": _hits(s.search(Q, CFG, filters=f)), "search_range": _hits(s.search_range(Q, threshold=0.2, filters=f)),
            "search_sessions": _hits(s.search_sessions(Q, CFG, filters=f)),
            "search_hybrid": _hits(s.search_hybrid("text 7 12 31", Q, CFG, filters=f)),
            "facets": [(fa.total, fa.missing, [(b.value, b.count, b.best.chunk_id, np.float32(b.best.similarity).tobytes())
                                               for b in fa.buckets])
                       for fa in (s.facets(Q, by=by, threshold=0.2, filters=f) for by in ("project_name", "has_code", "month"))]}


def _same(on, off, grid):
    for name, f in grid.items():
        a, b = _answers(on, f), _answers(off, f)
        assert a == b, name
        if name not in ("nothing passes",):
            assert a["search_range"], name                      # the filter leaves something to compare


def _spy(s):
    calls = []
    real = s._allow_mask
    s._allow_mask = lambda f, n: (calls.append(dict(f)), real(f, n))[1]
    return calls


def test_on_equals_off_over_the_filter_grid_tombstones_optimize_and_later_chunks(tmp_path):
    on, off = _pair(tmp_path, _chunks(0, 200))
    calls = _spy(on)
    _same(on, off, FILTERS)
    assert calls == []                                          # every filter of the grid compiled: no host loop
    assert on.faiss_index.attribute_type(0) == 0 and off.faiss_index.attribute_type(0) == -1
    # a timestamp range over chunks without a timestamp: the host comparison raises, in both
    for s in (on, off):
        with pytest.raises(TypeError):
            s.search(Q, CFG, filters=TS_FILTERS["timestamp range"])
    assert calls == [TS_FILTERS["timestamp range"]]             # declined ("a NULL under a range op"): the fallback ran
    del calls[:]
    # an uncompilable filter goes to the host loop and gives the same results
    assert _answers(on, UNCOMPILABLE) == _answers(off, UNCOMPILABLE) and _answers(on, UNCOMPILABLE)["search_range"]
    assert calls and all(c == UNCOMPILABLE for c in calls)
    del calls[:]
    # tombstones
    for s in (on, off):
        for i in (0, 6, 7, 100, 199):
            assert s.delete_chunk(f"c{i}")
    _same(on, off, FILTERS)
    # chunks appended later, with a project and a session not seen before: only the tail is pushed
    pushed = []
    real = on.faiss_index.set_attribute
    on.faiss_index.set_attribute = lambda slot, v, row0=0: (pushed.append((slot, row0, len(v))), real(slot, v, row0=row0))[1]
    late = _chunks(200, N) + [Chunk("late", "text late 7", {"project_name": "Alphabet", "session_id": "brand-new", "chunk_type": "code",
                                                             "has_code": True, "word_count": 61,
                                                             "timestamp": T0.isoformat()}, corpus(0, 1)[0].embedding)]
    for s in (on, off):
        s.add_chunks(copy.deepcopy(late))
    _same(on, off, FILTERS)
    assert any(r[0] == "late" for r in _answers(on, FILTERS["substring in the wrong case"])["search_range"])
    assert pushed and all(row0 == 200 for slot, row0, n in pushed if slot != 9)      # (slot 9: timestamps are re-ranked)
    del on.faiss_index.set_attribute
    # after optimize(): rows renumbered, the columns pushed again for the compacted index
    for s in (on, off):
        s.optimize()
    _same(on, off, FILTERS)
    assert calls == []
    # facets(by="project_name") reaches the index with buckets=None and by_attribute set
    seen = []
    real_facets = on.faiss_index.facets
    on.faiss_index.facets = lambda q, r, **kw: (seen.append(kw), real_facets(q, r, **kw))[1]
    on.facets(Q, by="project_name", threshold=0.2)
    on.facets(Q, by="month", threshold=0.2)
    assert seen[0]["buckets"] is None and seen[0]["by_attribute"] == 0
    assert seen[1]["buckets"] is not None and "by_attribute" not in seen[1]
    del on.faiss_index.facets
    for s in (on, off):
        s.close()


def test_on_equals_off_for_timestamp_ranges(tmp_path):
    on, off = _pair(tmp_path, _chunks(0, N, keep=lambda i: i % 10 != 9))
    calls = _spy(on)
    _same(on, off, TS_FILTERS)
    for s in (on, off):
        for i in (20, 33, 150):
            assert s.delete_chunk(f"c{i}")
    _same(on, off, TS_FILTERS)
    # chunks appended later: one whose timestamp sorts IN FRONT of stored ones (the ranks of every earlier row move and
    # the whole timestamp column is pushed again), one between stored values, one past them; a new project and session
    pushed = []
    real = on.faiss_index.set_attribute
    on.faiss_index.set_attribute = lambda slot, v, row0=0: (pushed.append((slot, row0, len(v))), real(slot, v, row0=row0))[1]
    e = corpus(0, 1)[0].embedding                                # similarity 0.9 to Q: inside every range search below
    late = [Chunk(f"late{j}", f"text late {j}", {"project_name": "Alphabet", "session_id": "brand-new", "chunk_type": "code",
                                                 "has_code": True, "word_count": 61 + j, "timestamp": ts}, e)
            for j, ts in enumerate(("2023-12-31T23:59:59", "2024-05-05T05:05:05", "2031-01-01T00:00:00Z", STAMP(21)))]
    rows = on.faiss_index.ntotal
    for s in (on, off):
        s.add_chunks(copy.deepcopy(late))
    _same(on, off, TS_FILTERS)
    assert (9, 0, rows + len(late)) in pushed                    # slot 9 = timestamp: re-ranked, pushed whole
    assert all(row0 == rows for slot, row0, n in pushed if slot != 9)
    del on.faiss_index.set_attribute
    got = _answers(on, TS_FILTERS["timestamp range, a bound between stored values"])["search_range"]
    assert any(r[0] == "late1" for r in got) and not any(r[0] in ("late0", "late2") for r in got)
    assert any(r[0] == "late3" for r in _answers(on, TS_FILTERS["timestamp exact"])["search_range"])
    front = {"timestamp": {"lt": "2024"}, "project_name": "alphab"}      # only the chunk that sorts in front
    assert _answers(on, front) == _answers(off, front) and [r[0] for r in _answers(on, front)["search_range"]] == ["late0"]
    # after optimize(): rows renumbered, a new catalog, the ranks rebuilt over the compacted rows
    for s in (on, off):
        s.optimize()
    _same(on, off, TS_FILTERS)
    assert _answers(on, front) == _answers(off, front) and [r[0] for r in _answers(on, front)["search_range"]] == ["late0"]
    for s in (on, off):
        assert s.delete_chunk("late0")
    _same(on, off, TS_FILTERS)
    assert _answers(on, front) == _answers(off, front) and _answers(on, front)["search_range"] == []
    assert calls == []
    for s in (on, off):
        s.close()
