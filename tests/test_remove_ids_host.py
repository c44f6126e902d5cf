"""CPU: compaction of tombstones through ``remove_ids`` (HybridStorage host logic) and the keep-mask helper of
``IndexFlat.remove_ids``.  The device index is replaced by a numpy TEST DOUBLE that lives in this file only; one
variant of it offers ``remove_ids`` (the in-place path of ``_rebuild_faiss_index``), the other does not (the rebuild
into a second index, unchanged)."""
import shutil
import tempfile
from pathlib import Path

import numpy as np
import pytest

from oracle import knn_oracle as ko
from claude_semantic_search_amd import flat_index as fi
from claude_semantic_search_amd.chunk import Chunk
from claude_semantic_search_amd.storage import HybridStorage, StorageConfig

D = 8
EVENTS = []   # (what, payload) of every index constructed / add / remove_ids, in order


class _RebuildOnlyIndex:
    """numpy flat index without remove_ids."""

    def __init__(self, d, metric=0, device=0):
        self.d, self.metric_type, self.device = int(d), int(metric), device
        self._x = np.zeros((0, self.d), np.float32)
        EVENTS.append(("construct", None))

    ntotal = property(lambda self: self._x.shape[0])

    def add(self, x, normalize=False):
        x = np.asarray(x, np.float32).reshape(-1, self.d)
        EVENTS.append(("add", x.shape[0]))
        self._x = np.concatenate([self._x, ko.normalize_rows(x) if normalize else x])

    def search(self, q, k, normalize=False, allow=None):
        q = np.asarray(q, np.float32).reshape(-1, self.d)
        q = ko.normalize_rows(q) if normalize else q
        sub = np.arange(self.ntotal) if allow is None else np.flatnonzero(np.asarray(allow, dtype=bool))
        o = ko.FlatIndexOracle(self.d, self.metric_type)
        if sub.size:
            o.add(self._x[sub])
        Dm, I = o.search(q, k)
        return Dm, np.where(I >= 0, sub[np.clip(I, 0, max(sub.size - 1, 0))] if sub.size else -1, -1)

    def reconstruct_n(self, row0=0, n=None):
        n = self.ntotal - row0 if n is None else n
        return self._x[row0:row0 + n].copy()

    def reserve(self, n):
        pass

    def reset(self):
        self._x = self._x[:0]

    def close(self):
        pass


class _RemovingIndex(_RebuildOnlyIndex):
    """The same, with faiss' remove_ids."""

    def remove_ids(self, ids):
        keep = fi.keep_mask_from_ids(ids, self.ntotal)
        EVENTS.append(("remove_ids", np.flatnonzero(~keep).tolist()))
        removed = int((~keep).sum())
        self._x = self._x[keep]
        return removed


def _install(monkeypatch, cls):
    monkeypatch.setattr(fi, "IndexFlat", cls)
    monkeypatch.setattr(fi, "IndexFlatIP", lambda d, device=0: cls(d, 0, device))
    monkeypatch.setattr(fi, "IndexFlatL2", lambda d, device=0: cls(d, 1, device))


def _chunks(n=12):
    rng = np.random.default_rng(11)
    v = ko.normalize_rows(rng.standard_normal((n, D)).astype(np.float32))
    return [Chunk(f"c{i:02d}", f"text {i}", {"session_id": f"s{i % 3}", "project_name": "p"}, v[i].tolist())
            for i in range(n)], v


DEAD = [0, 4, 5, 11]   # first row, a run in the middle, last row


class _Scenario:
    def __init__(self):
        self.tmp = tempfile.mkdtemp()
        self.config = StorageConfig(data_dir=self.tmp, embedding_dim=D, auto_save=False)
        self.storage = HybridStorage(self.config)
        self.chunks, self.v = _chunks()
        self.storage.initialize()
        self.storage.add_chunks(self.chunks)
        self.v = self.storage.faiss_index.reconstruct_n(0, len(self.chunks))   # as stored (normalised once more)
        self.storage.save_index()
        for i in DEAD:
            assert self.storage.delete_chunk(f"c{i:02d}")
        self.live = [i for i in range(len(self.chunks)) if i not in DEAD]

    def close(self):
        try:
            self.storage.close()
        except Exception:
            pass
        shutil.rmtree(self.tmp, ignore_errors=True)

    def check_storage(self, s, n_rows, compacted):
        """ids, rows and hits of a storage whose index holds n_rows rows."""
        assert s.total_chunks == len(self.live) and s.faiss_index.ntotal == n_rows
        rows = s.db.execute("SELECT id, faiss_id FROM chunks WHERE faiss_id IS NOT NULL ORDER BY faiss_id").fetchall()
        assert [r["id"] for r in rows] == [f"c{i:02d}" for i in self.live]
        assert [r["faiss_id"] for r in rows] == (list(range(len(self.live))) if compacted else self.live)
        for r in rows:   # every id points at its own vector
            assert np.array_equal(s.faiss_index.reconstruct_n(r["faiss_id"], 1)[0], self.v[int(r["id"][1:])])
        for i in self.live:
            hits = s.search(self.v[i])
            assert hits[0].chunk_id == f"c{i:02d}" and abs(hits[0].similarity - 1.0) < 1e-5
            assert not {h.chunk_id for h in hits} & {f"c{j:02d}" for j in DEAD}

    def check_reopened(self, n_rows, compacted):
        other = HybridStorage(self.config)
        other.initialize()
        self.check_storage(other, n_rows, compacted)
        assert not Path(str(other.index_path) + ".compact").exists()
        assert other.db.execute("SELECT COUNT(*) FROM storage_meta WHERE key = 'pending_compact'").fetchone()[0] == 0
        other.close()


@pytest.fixture
def scenario(monkeypatch, request):
    _install(monkeypatch, request.param)
    sc = _Scenario()
    EVENTS.clear()
    yield sc
    sc.close()


@pytest.mark.parametrize("scenario", [_RemovingIndex], indirect=True)
def test_optimize_compacts_in_place_through_remove_ids(scenario):
    sc = scenario
    index_before = sc.storage.faiss_index
    sc.storage.optimize()
    assert [e for e in EVENTS if e[0] == "remove_ids"] == [("remove_ids", DEAD)]   # once, exactly the tombstones
    assert not [e for e in EVENTS if e[0] in ("construct", "add")]                  # no second index, no re-add
    assert sc.storage.faiss_index is index_before
    sc.check_storage(sc.storage, len(sc.live), compacted=True)
    # the index file holds the compacted rows already (no save_index(), no close())
    EVENTS.clear()
    back = fi.read_index(str(sc.storage.index_path))
    assert back.ntotal == len(sc.live) and np.array_equal(back.reconstruct_n(0, back.ntotal), sc.v[sc.live])
    ref = _RebuildOnlyIndex(D, 0)
    ref.add(sc.v[sc.live])
    fi.write_index(ref, str(Path(sc.tmp) / "ref.faiss"))
    assert sc.storage.index_path.read_bytes() == (Path(sc.tmp) / "ref.faiss").read_bytes()
    sc.check_reopened(len(sc.live), compacted=True)
    # and the storage goes on working: append, delete, compact again
    extra = Chunk("c99", "more", {"session_id": "s9", "project_name": "p"}, sc.v[0].tolist())
    sc.storage.add_chunks([extra])
    assert sc.storage.search(sc.v[0])[0].chunk_id == "c99"
    assert sc.storage.delete_chunk("c01")
    sc.storage.optimize()
    assert sc.storage.faiss_index.ntotal == len(sc.live) and sc.storage.search(sc.v[0])[0].chunk_id == "c99"


@pytest.mark.parametrize("scenario", [_RemovingIndex], indirect=True)
def test_interrupted_in_place_compaction_leaves_the_live_index_alone(scenario):
    """Both crash windows of the journal: the id update fails after the compacted file was written, and the process
    dies between the commit and the rename.  In both the live index must not have been compacted, and the data_dir
    must open to a state in which ids and rows match."""
    sc = scenario

    class Crash(Exception):
        pass

    real_write = HybridStorage._write_index_atomically

    def write_then_die(ix, path):
        real_write(ix, path)
        if path.endswith(".compact"):
            raise Crash()

    sc.storage._write_index_atomically = write_then_die
    with pytest.raises(Crash):
        sc.storage.optimize()
    sc.storage.db.rollback()
    del sc.storage._write_index_atomically
    assert not [e for e in EVENTS if e[0] == "remove_ids"]
    assert Path(str(sc.storage.index_path) + ".compact").exists()
    sc.check_storage(sc.storage, len(sc.chunks), compacted=False)    # memory: old rows + old ids
    sc.check_reopened(len(sc.chunks), compacted=False)               # disk: old file + old ids, leftover removed

    def die(where):
        raise Crash(where)

    sc.storage._crash_point = die
    with pytest.raises(Crash):
        sc.storage.optimize()
    assert not [e for e in EVENTS if e[0] == "remove_ids"]
    assert sc.storage.faiss_index.ntotal == len(sc.chunks)
    assert np.array_equal(sc.storage.faiss_index.reconstruct_n(0, len(sc.chunks)), sc.v)
    sc.check_reopened(len(sc.live), compacted=True)                  # recovery moved the compacted file into place
    sc.check_reopened(len(sc.live), compacted=True)


@pytest.mark.parametrize("scenario", [_RebuildOnlyIndex], indirect=True)
def test_index_without_remove_ids_is_rebuilt_as_before(scenario):
    sc = scenario
    index_before = sc.storage.faiss_index
    sc.storage.optimize()
    assert [e[0] for e in EVENTS if e[0] != "add"] == ["construct"] and ("add", len(sc.live)) in EVENTS
    assert sc.storage.faiss_index is not index_before
    sc.check_storage(sc.storage, len(sc.live), compacted=True)
    sc.check_reopened(len(sc.live), compacted=True)


def test_keep_mask_from_ids():
    n = 70
    ids = [3, 69, 0, 3, 3, 70, -1, 10 ** 12, 33]
    keep = fi.keep_mask_from_ids(ids, n)
    want = np.ones(n, bool)
    want[[0, 3, 33, 69]] = False
    assert keep.dtype == np.bool_ and np.array_equal(keep, want)
    assert int((~keep).sum()) == 4                                     # repeated / out-of-range ids are not counted
    assert np.array_equal(fi.keep_mask_from_ids(~want, n), want)      # mask form: True = remove
    for same in (np.array(ids, np.int64), tuple(ids), np.array([0, 3, 33, 69], np.int32), np.array([69, 3, 33, 0], np.uint64)):
        assert np.array_equal(fi.keep_mask_from_ids(same, n), want)
    assert fi.keep_mask_from_ids([], n).all() and fi.keep_mask_from_ids(np.zeros(0, np.int64), n).all()
    assert fi.keep_mask_from_ids(np.zeros(n, bool), n).all() and not fi.keep_mask_from_ids(np.ones(n, bool), n).any()
    assert fi.keep_mask_from_ids([], 0).shape == (0,)
    for bad in (np.zeros(n - 1, bool), np.zeros(n + 1, bool), np.zeros((n, 1), bool)):
        with pytest.raises(ValueError):
            fi.keep_mask_from_ids(bad, n)
    for bad in ([1.0, 2.0], np.array([1.5]), ["3"], np.array([1 + 0j])):
        with pytest.raises(ValueError):
            fi.keep_mask_from_ids(bad, n)
    # the bitmap handed to the library: bit (r & 31) of word r >> 5 set = the row stays
    bits = fi.pack_allow_bits(keep, n)
    assert bits.shape == (3,) and [(int(bits[r >> 5]) >> (r & 31)) & 1 for r in range(n)] == want.astype(int).tolist()
