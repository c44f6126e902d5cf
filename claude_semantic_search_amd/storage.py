"""``HybridStorage``: flat vector index in MI355X HBM + SQLite metadata.

Drop-in for the reference's ``src/storage.py`` (same public names, argument
meaning and error behaviour) with the faiss calls replaced by
``flat_index`` (libcss_hip.so).  Numeric path, reference file:line:

  * metric choice: ``normalize_embeddings`` -> inner product, else squared L2
    (``src/storage.py:252-258``); unknown ``index_type`` -> ``ValueError``
    (``:267``); "ivf"/"hnsw" are not reachable from the product and are not
    implemented here.
  * ``add_chunks``: float32 cast, ``x / (||x|| + 1e-8)``, ids = ntotal.. (``:343-365``)
    -- the normalisation is fused into the device ingest kernel.
  * ``search``: query normalise, ``k' = min(max_results, ntotal)``, top-k'
    (``:424-436``), then threshold / tombstone skip / SQLite row / filters /
    stop at ``top_k`` in rank order (``:438-492``).

Deliberate differences (all on the host side of the kernel):
  * nothing touches the GPU before ``initialize()`` (fork safety);
  * a lock serialises index/id-map mutation against searches (the reference has none);
  * ``auto_save`` appends the new rows to ``embeddings.faiss`` instead of
    rewriting the whole file after every add (the reference's O(N^2) I/O);
  * there is no CPU index: without a HIP device ``initialize()`` raises;
  * opt-in ``StorageConfig.filter_pushdown``: filters / tombstones become an allow-bitmap consumed by the
    kernel (``css_index_search_masked``) instead of an over-fetch of ``max_results`` hits.
"""
from __future__ import annotations

import json
import logging
import os
import sqlite3
import struct
import threading
from dataclasses import dataclass
from datetime import datetime, timezone
from pathlib import Path
from typing import Any, Callable, Dict, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

from . import flat_index as fi
from .chunk import Chunk
from .filters import ATTR_COLUMNS, DICT_COLUMNS, FLAG_COLUMNS, AttrCatalog, compile_filters
from .gpu_utils import GPUCapability, assess_gpu_capability, log_gpu_status

# bytes in front of the row data of faiss' IndexFlat file: fourcc, d, ntotal, 2 dummies, is_trained, metric, n_floats
_INDEX_HEADER_BYTES = 4 + 4 + 8 + 16 + 1 + 4 + 8


@dataclass
class StorageConfig:
    data_dir: str = "~/.claude-semantic-search/data"
    db_name: str = "metadata.db"
    index_name: str = "embeddings.faiss"
    embedding_dim: int = 768
    index_type: str = "flat"  # only "flat" is implemented
    ivf_nlist: int = 100
    hnsw_m: int = 16
    normalize_embeddings: bool = True
    auto_save: bool = True
    backup_enabled: bool = True
    use_gpu: bool = False
    gpu_memory_fraction: float = 0.8
    device: int = 0  # HIP device ordinal holding the index (extension)
    # extension: push filters and tombstones down into the kNN kernel as an allow-bitmap, so a
    # filtered search returns the true filtered top_k instead of whatever survives inside the first
    # ``max_results`` unfiltered hits.  Off by default: the reference's over-fetch semantics are kept bit for bit.
    filter_pushdown: bool = False
    # extension (the reference pins faiss to one device, src/storage.py:283): row-shard the index over the
    # ranks of the default torch.distributed process group, one process per GPU.  SPMD: every rank constructs the same
    # HybridStorage (its own data_dir: SQLite and the index file are replicated per rank) and makes the same calls
    # with the same arguments; search() is then the local masked search of every shard + ONE all-gather + merge.
    # CSS_STORAGE_SHARDED=1 switches it on for an unmodified caller (the reference's CLI under torch.distributed.run).
    sharded: bool = False
    # extension: evaluate filters on the GPU.  The filterable chunk columns are kept as attribute columns of the index
    # (``IndexFlat.set_attribute``) and a filter dict is compiled into ``IndexFlat.where`` clauses (``filters.py``); a
    # filter that cannot be compiled with exactly the host's semantics falls back to the host loop.  It changes where
    # the allow mask of a search is computed, never what a search returns.  Off by default.
    attribute_filters: bool = False
    # extension: store the chunks' token matrices (index_tokens / search_late) COMPRESSED, ColBERTv2's residual codec:
    # a token is the id of its nearest centroid plus ``token_codec_bits`` (1, 2 or 4) per component -- 2 + P bits / 8
    # bytes in place of 2 P.  The codec is trained on the first batch of encoded chunks with at most
    # ``token_codec_centroids`` centroids (<= 4096).  0 = off: the matrices are stored as they are.
    token_codec_bits: int = 0
    token_codec_centroids: int = 4096
    # Candidates of ``search_late`` on an index with a token codec: the chunks are first ranked by the MaxSim of their
    # tokens' centroids (2 bytes per token read) and only the best ``late_candidates`` are decoded and scored exactly
    # (``IndexFlat.search_maxsim_pruned``, PLAID's centroid interaction).  0 = exhaustive: every allowed chunk is scored.
    late_candidates: int = 0


@dataclass
class SearchConfig:
    top_k: int = 10
    similarity_threshold: float = 0.0
    include_metadata: bool = True
    include_text: bool = True
    max_results: int = 100


@dataclass
class SearchResult:
    chunk_id: str
    similarity: float
    chunk: Optional[Chunk] = None
    metadata: Optional[Dict[str, Any]] = None
    text: Optional[str] = None


class Reranked(NamedTuple):
    """One hit of ``HybridStorage.search_reranked``: the plain search result, the cross-encoder logit of
    ``(query_text, chunk text)`` and the chunk's position in the plain search's ranking (0 = its best hit)."""
    result: SearchResult
    score: float
    rank_before: int


@dataclass
class Topic:
    """One cluster of ``HybridStorage.topics``: its number of live chunks, the chunk nearest its centroid, the nearest
    few chunks (``representative`` is ``examples[0]``; similarities are to the centroid) and the ids of all members."""
    size: int
    representative: SearchResult
    examples: List[SearchResult]
    chunk_ids: List[str]


@dataclass
class Keyword:
    """One term of ``HybridStorage.keywords``: the word, its hashed term id, the number of selected chunks and of live
    chunks that hold it, and its JLH score."""
    word: str
    term: int
    count: int
    background_count: int
    score: float


@dataclass
class Facet:
    """One bucket of ``HybridStorage.facets``: the value the chunks share (a column value, or the ISO date of the first
    day of a day / week / month), the number of matching chunks, and the best of them."""
    value: Any
    count: int
    best: SearchResult


@dataclass
class Facets:
    """What ``HybridStorage.facets`` returns: all matching chunks, those among them without a value for the facet
    (``missing``), and the non-empty buckets, largest first."""
    total: int
    missing: int
    buckets: List[Facet]


@dataclass
class MapPoint:
    """One chunk of ``HybridStorage.map``: its coordinates on the first two principal components of the selection, and
    its k-means topic under the same selection (``None`` when no topics were asked for)."""
    chunk_id: str
    x: float
    y: float
    topic: Optional[int] = None


_CHUNK_COLUMNS = (
    "id", "text", "metadata", "faiss_id", "session_id", "project_name", "file_path", "chunk_type",
    "timestamp", "has_code", "has_tools", "message_count", "char_count", "word_count", "updated_at",
)

_SCHEMA = (
    """CREATE TABLE IF NOT EXISTS chunks (
        id TEXT PRIMARY KEY, text TEXT NOT NULL, metadata TEXT, faiss_id INTEGER,
        session_id TEXT, project_name TEXT, file_path TEXT, chunk_type TEXT, timestamp DATETIME,
        has_code BOOLEAN, has_tools BOOLEAN, message_count INTEGER, char_count INTEGER, word_count INTEGER,
        created_at DATETIME DEFAULT CURRENT_TIMESTAMP, updated_at DATETIME DEFAULT CURRENT_TIMESTAMP)""",
    """CREATE TABLE IF NOT EXISTS files (
        path TEXT PRIMARY KEY, last_modified DATETIME, last_indexed DATETIME, chunk_count INTEGER DEFAULT 0)""",
    "CREATE INDEX IF NOT EXISTS idx_chunks_session ON chunks(session_id)",
    "CREATE INDEX IF NOT EXISTS idx_chunks_project ON chunks(project_name)",
    "CREATE INDEX IF NOT EXISTS idx_chunks_timestamp ON chunks(timestamp)",
    "CREATE INDEX IF NOT EXISTS idx_chunks_type ON chunks(chunk_type)",
    "CREATE INDEX IF NOT EXISTS idx_chunks_has_code ON chunks(has_code)",
    "CREATE INDEX IF NOT EXISTS idx_chunks_has_tools ON chunks(has_tools)",
    "CREATE INDEX IF NOT EXISTS idx_chunks_faiss_id ON chunks(faiss_id)",
    # build-owned: journal of the two-file operations (index file + SQLite) that must survive a crash between them
    "CREATE TABLE IF NOT EXISTS storage_meta (key TEXT PRIMARY KEY, value TEXT)",
)


def _fsync_dir(path: Path) -> None:
    """Make a rename inside ``path`` durable (POSIX: fsync of the directory; skipped where a directory cannot be opened)."""
    try:
        fd = os.open(str(path), os.O_RDONLY)
    except OSError:
        return
    try:
        os.fsync(fd)
    except OSError:
        pass
    finally:
        os.close(fd)


def _row_to_chunk(row) -> Chunk:
    meta = json.loads(row["metadata"]) if row["metadata"] else {}
    return Chunk(id=row["id"], text=row["text"], metadata=meta, embedding=None)


class _LiveRows:
    """The live rows of an index, seen as an index of their own by ``flat_index.write_index``: row ``i`` is row
    ``ids[i]`` of ``index`` (``ids`` ascending).  Rows are exported run by run; nothing is copied into a second index."""

    def __init__(self, index, ids):
        self._index = index
        self._ids = np.asarray(ids, dtype=np.int64)
        self.d, self.metric_type, self.ntotal = index.d, index.metric_type, int(self._ids.shape[0])

    def reconstruct_n(self, row0: int, n: int) -> np.ndarray:
        out = np.empty((n, self.d), dtype=np.float32)
        step = 1 << 16
        for s in range(0, n, step):
            part = self._ids[row0 + s:row0 + min(s + step, n)]
            lo, hi = int(part[0]), int(part[-1]) + 1
            out[s:s + part.shape[0]] = self._index.reconstruct_n(lo, hi - lo)[part - lo]
        return out


# search_recent: the largest exponent of 2 a stored prior or the call's weight factor may carry (fp32 holds 2^127;
# 60 leaves the fused value far from overflow and the priors far from underflow for every half-life in between)
RECENCY_MAX_EXPONENT = 60.0


def recency_priors(t_days, t_ref_days: float, half_life_days: float) -> np.ndarray:
    """The stored per-row prior of ``search_recent``: ``p_r = 2^((t_r - t_ref) / h)`` as float32, for timestamps
    ``t_days`` (days on any common clock; NaN = no timestamp -> prior 0, infinitely old).  The column does not depend
    on "now": a search at time ``now`` passes ``weight * 2^(-(now - t_ref) / h)`` as the call's weight, and the
    product is ``weight * 2^(-age / h)``.  Exponents beyond ``RECENCY_MAX_EXPONENT`` raise ``ValueError``: the caller
    re-references first (``t_ref`` = the newest timestamp, which makes every exponent <= 0)."""
    h = float(half_life_days)
    if not (h > 0.0) or not np.isfinite(h):
        raise ValueError(f"half_life_days={half_life_days} must be a positive finite number")
    t = np.asarray(t_days, dtype=np.float64).reshape(-1)
    e = (t - float(t_ref_days)) / h
    known = ~np.isnan(e)
    if known.any() and float(e[known].max()) > RECENCY_MAX_EXPONENT:
        raise ValueError(f"recency_priors: exponent {float(e[known].max()):.1f} beyond {RECENCY_MAX_EXPONENT:.0f}: "
                         "re-reference t_ref to the newest timestamp")
    out = np.zeros(t.shape[0], dtype=np.float32)
    with np.errstate(under="ignore"):
        out[known] = np.exp2(e[known]).astype(np.float32)
    return out


def timestamp_days(ts) -> float:
    """A chunk's ``timestamp`` column (ISO string or ``datetime``; naive = UTC) as days since the Unix epoch; NaN for
    a missing or unparseable one."""
    if ts is None:
        return float("nan")
    try:
        if not isinstance(ts, datetime):
            text = str(ts).strip()
            if text.endswith(("Z", "z")):
                text = text[:-1] + "+00:00"
            ts = datetime.fromisoformat(text)
        if ts.tzinfo is None:
            ts = ts.replace(tzinfo=timezone.utc)
        return ts.timestamp() / 86400.0
    except (ValueError, OverflowError, OSError):
        return float("nan")


def strict_radius(threshold: float, similarity: bool) -> np.float32:
    """The float32 radius that makes the index's STRICT comparison mean ``>= threshold`` (``similarity``: inner
    product, ``score > radius``) or ``<= threshold`` (squared L2, ``dist < radius``) for every float32 score: the
    float32 next to the threshold on the far side.  ``search_range`` and ``facets`` share it."""
    thr = float(threshold)
    with np.errstate(over="ignore"):   # (a threshold beyond float32 ends at +-inf, which is the right radius)
        t32 = np.float32(thr)
        if similarity:
            # score >= thr  <=>  score >= (smallest float32 >= thr)  <=>  score > the float32 below that one
            if float(t32) < thr:
                t32 = np.nextafter(t32, np.float32(np.inf))
            return np.nextafter(t32, np.float32(-np.inf))
        if float(t32) > thr:
            t32 = np.nextafter(t32, np.float32(-np.inf))
        return np.nextafter(t32, np.float32(np.inf))


FACET_COLUMNS = ("project_name", "session_id", "chunk_type", "has_code", "has_tools")
FACET_DATES = ("day", "week", "month")


def facet_date_key(days: float, by: str) -> Optional[int]:
    """The bucket of a timestamp (``timestamp_days``; NaN: ``None``) under ``by`` = day / week / month, as an integer:
    the floored day number, the day number of the week's Monday, or ``year * 12 + month - 1`` (all UTC)."""
    if days != days:
        return None
    day = int(np.floor(days))
    if by == "day":
        return day
    if by == "week":
        return (day + 3) // 7 * 7 - 3   # (day 0, 1970-01-01, was a Thursday)
    d = datetime.fromtimestamp(day * 86400.0, tz=timezone.utc)
    return d.year * 12 + d.month - 1


def facet_date_value(key: int, by: str) -> str:
    """The ISO date of the first day of the bucket ``facet_date_key`` named."""
    if by == "month":
        return f"{key // 12:04d}-{key % 12 + 1:02d}-01"
    return datetime.fromtimestamp(key * 86400.0, tz=timezone.utc).date().isoformat()


def order_facets(buckets: List[Facet], similarity: bool, top: Optional[int] = None) -> List[Facet]:
    """The order of ``HybridStorage.facets``: count descending, then the better best hit (``similarity``: larger;
    squared distance: smaller), then the value; cut to ``top`` when given."""
    out = sorted(buckets, key=lambda f: (-f.count, -f.best.similarity if similarity else f.best.similarity, f.value))
    return out if top is None else out[:max(int(top), 0)]


class _Synced:
    """Which rows of WHICH index object already carry a per-row column that is pushed lazily, in front of the search
    that reads it (session labels, recency priors, term lists).  A fresh one is synced with no index."""

    index: Optional[Any] = None
    rows = 0

    def rows_of(self, index) -> int:
        """Rows of ``index`` that carry the column; another object than last time is adopted with none."""
        if self.index is not index:
            self.index, self.rows = index, 0
        return self.rows


class HybridStorage:
    def __init__(self, config: Optional[StorageConfig] = None) -> None:
        self.config: StorageConfig = config or StorageConfig()
        self.logger = logging.getLogger(__name__)
        self.data_dir: Path = Path(self.config.data_dir).expanduser()
        self.data_dir.mkdir(parents=True, exist_ok=True)
        self.db_path: Path = self.data_dir / self.config.db_name
        self.index_path: Path = self.data_dir / self.config.index_name

        self.db: Optional[sqlite3.Connection] = None
        self.faiss_index: Optional[fi.IndexFlat] = None
        self.chunk_id_to_faiss_id: Dict[str, int] = {}
        self.faiss_id_to_chunk_id: Dict[int, str] = {}

        self._gpu_capability: Optional[GPUCapability] = None
        self._gpu_resources: Optional[Any] = None
        self._is_gpu_index: bool = False
        self._lock = threading.RLock()
        self._saved_rows = -1  # rows known to be in index_path (-1: unknown)
        self._allow_cache: Dict[str, Any] = {}  # filter key -> (stamp, allow mask); push-down only
        self._facet_cache: Dict[str, Any] = {}  # facets: by -> (stamp, bucket ids, values)
        self._mutations = 0  # bumped by every change of the chunk set (part of the allow-cache stamp)
        # the lazily pushed columns of search_sessions (labels), search_recent (priors) and search_hybrid (term lists)
        self._labels, self._priors, self._terms = _Synced(), _Synced(), _Synced()
        # index_sparse / search_sparse: the rows that carry a sparse vector, the model that made the vectors, and what
        # of them the file beside the index holds as (model, rows with a vector, rows of the index)
        self._sparse = _Synced()
        # attribute_filters: the chunk columns pushed into attribute slots, and what their codes mean
        self._attrs = _Synced()
        self._catalog = AttrCatalog()
        self._live_cache: Optional[Tuple[Any, np.ndarray]] = None
        self._sparse_model: Optional[str] = None
        self._sparse_saved: Optional[Tuple[Optional[str], int, int]] = None
        # index_tokens / search_late: the same three for the chunks' token matrices (late interaction)
        self._tokens = _Synced()
        self._tokens_model: Optional[str] = None
        self._tokens_saved: Optional[Tuple[Optional[str], int, int]] = None
        self._tokens_codec_model: Optional[str] = None   # the model whose tokens the index's token codec was trained on
        # search_sessions: dense group labels per session_id (order of first appearance by faiss_id)
        self._session_labels: Dict[str, int] = {}
        # search_recent: the half-life and reference time (days since the epoch) the priors are stored for; the newest
        # timestamp seen so far
        self._priors_half_life: Optional[float] = None
        self._priors_t_ref: Optional[float] = None
        self._priors_newest: Optional[float] = None

        self.total_chunks: int = 0
        self.embedding_dim: int = self.config.embedding_dim

    # ------------------------------------------------------------ lifecycle
    def initialize(self) -> None:
        self.logger.info("Initializing hybrid storage...")
        with self._lock:
            self._init_sqlite()
            self._init_faiss()
            self._load_existing_data()
        self.logger.info(f"Storage initialized with {self.total_chunks} chunks")

    def _init_sqlite(self) -> None:
        self.db = sqlite3.connect(str(self.db_path), check_same_thread=False)
        self.db.row_factory = sqlite3.Row
        self._create_tables()

    def _create_tables(self) -> None:
        if not self.db:
            raise RuntimeError("Database not initialized")
        cur = self.db.cursor()
        for stmt in _SCHEMA:
            cur.execute(stmt)
        self.db.commit()

    def _create_cpu_index(self) -> fi.IndexFlat:
        """Name kept from the reference; the index is created in HBM."""
        kind = self.config.index_type
        if kind == "flat":
            if self._sharded():
                from .sharded import ShardedIndexFacade

                metric = fi.METRIC_INNER_PRODUCT if self.config.normalize_embeddings else fi.METRIC_L2
                return ShardedIndexFacade(self.embedding_dim, metric, device=self.config.device)
            cls = fi.IndexFlatIP if self.config.normalize_embeddings else fi.IndexFlatL2
            return cls(self.embedding_dim, device=self.config.device)
        if kind in ("ivf", "hnsw"):
            raise NotImplementedError(
                f"index type {kind!r} is not reachable from the product and is not implemented on MI355X; use 'flat'"
            )
        raise ValueError(f"Unknown index type: {kind}")

    def _sharded(self) -> bool:
        return bool(self.config.sharded) or os.environ.get("CSS_STORAGE_SHARDED") == "1"

    def _read_index(self, path: str):
        if self._sharded():
            from .sharded import read_index_sharded

            return read_index_sharded(path, device=self.config.device)
        return fi.read_index(path, device=self.config.device)

    def _init_faiss(self) -> None:
        if self.config.use_gpu and self._gpu_capability is None:
            # assessed here, not in __init__, so no HIP context exists before a fork
            self._gpu_capability = assess_gpu_capability()
            if not self._gpu_capability.can_use_gpu:
                self.logger.warning(f"GPU requested but not available: {self._gpu_capability.status_message}")
        self.faiss_index = self._create_cpu_index()
        self._is_gpu_index = True
        self._saved_rows = -1
        self.logger.info(f"Initialized HIP flat index: {type(self.faiss_index).__name__} on device {self.config.device}")
        if self._gpu_capability:
            log_gpu_status(self._gpu_capability, self.logger)

    def _convert_to_gpu_index(self, cpu_index):
        return fi.index_cpu_to_gpu(self._gpu_resources, self.config.device, cpu_index)

    def _convert_to_cpu_index(self, gpu_index):
        return fi.index_gpu_to_cpu(gpu_index)

    def _recover_interrupted_compaction(self) -> None:
        """Finish or discard a compaction (``_rebuild_faiss_index``) that a crash interrupted.  Its order is:
        (1) compacted rows -> ``<index>.compact``; (2) ONE SQLite transaction renumbers the ids and sets
        ``storage_meta['pending_compact']``; (3) ``os.replace(<index>.compact, <index>)``; (4) the flag is cleared.
        So: flag set -> SQLite already speaks the new numbering and the compacted file is either still beside the
        index (finish step 3) or already in place; flag absent -> a leftover ``.compact`` was never committed."""
        compact = Path(str(self.index_path) + ".compact")
        row = self.db.execute("SELECT value FROM storage_meta WHERE key = 'pending_compact'").fetchone()
        if row is not None:
            self._drop_sparse_file()   # (the sparse vectors beside the index speak the old numbering)
            self._drop_tokens_file()   # (and so do the token matrices)
            if compact.exists():
                os.replace(str(compact), str(self.index_path))
                _fsync_dir(self.index_path.parent)
                self.logger.warning("Completed an interrupted index compaction (compacted file moved into place)")
            self.db.execute("DELETE FROM storage_meta WHERE key = 'pending_compact'")
            self.db.commit()
        elif compact.exists():
            compact.unlink()
            self.logger.warning("Removed the leftover of an index compaction that never committed")

    def _load_existing_data(self) -> None:
        self._recover_interrupted_compaction()
        if not self.index_path.exists():
            return
        try:
            loaded = self._read_index(str(self.index_path))
            if loaded.d != self.embedding_dim:
                raise RuntimeError(f"index file has d={loaded.d}, expected {self.embedding_dim}")
            self.faiss_index = loaded
            self._saved_rows = loaded.ntotal
            self.logger.info(f"Loaded flat index with {loaded.ntotal} vectors")
            self._rebuild_id_mappings()
            self._load_sparse()
            self._load_tokens()
            bad = [i for i in self.faiss_id_to_chunk_id if i >= loaded.ntotal]
            if bad:   # e.g. a crash before the last save with auto_save off: those chunks have no vector on file
                self.logger.warning(f"{len(bad)} chunks refer to rows beyond the {loaded.ntotal} rows of the index file; "
                                    "they cannot be returned by searches until they are re-indexed")
        except Exception as e:  # corrupt / foreign file -> fresh index (src/storage.py:314-316)
            self.logger.warning(f"Could not load existing FAISS index: {e}")
            self._init_faiss()

    def _rebuild_id_mappings(self) -> None:
        self._mutations += 1  # invalidates cached allow masks (filter push-down)
        cur = self.db.cursor()
        cur.execute("SELECT id, faiss_id FROM chunks WHERE faiss_id IS NOT NULL")
        fwd: Dict[str, int] = {}
        rev: Dict[int, str] = {}
        for chunk_id, faiss_id in cur.fetchall():
            fwd[chunk_id] = faiss_id
            rev[faiss_id] = chunk_id
        self.chunk_id_to_faiss_id.update(fwd)
        self.faiss_id_to_chunk_id.update(rev)
        self.total_chunks = len(self.chunk_id_to_faiss_id)
        self.logger.info(f"Rebuilt ID mappings for {self.total_chunks} chunks")

    # ------------------------------------------------------------------ add
    def add_chunks(self, chunks: List[Chunk]) -> None:
        self._mutations += 1  # invalidates cached allow masks (filter push-down)
        if not chunks:
            return
        with_emb = [c for c in chunks if c.embedding is not None]
        if not with_emb:
            self.logger.warning("No chunks with embeddings to add")
            return
        if all(isinstance(c.embedding, np.ndarray) for c in with_emb):
            x = np.stack([c.embedding for c in with_emb]).astype(np.float32, copy=False)  # EmbeddingConfig.embeddings_as_arrays
        else:
            x = np.array([c.embedding for c in with_emb], dtype=np.float32)
        if not self.faiss_index:
            raise RuntimeError("FAISS index not initialized")
        if not self.db:
            raise RuntimeError("Database not initialized")
        with self._lock:
            first_id = self.faiss_index.ntotal
            # x / (||x|| + 1e-8) happens inside the ingest kernel when requested
            self.faiss_index.add(x, normalize=self.config.normalize_embeddings)
            now = datetime.now().isoformat()
            rows = []
            for off, chunk in enumerate(with_emb):
                fid = first_id + off
                self.chunk_id_to_faiss_id[chunk.id] = fid
                self.faiss_id_to_chunk_id[fid] = chunk.id
                md = chunk.metadata
                rows.append(
                    (chunk.id, chunk.text, json.dumps(md), fid, md.get("session_id"), md.get("project_name"),
                     md.get("file_path"), md.get("chunk_type"), md.get("timestamp"), md.get("has_code", False),
                     md.get("has_tools", False), md.get("message_count", 0), md.get("char_count", 0),
                     md.get("word_count", 0), now)
                )
            marks = ", ".join("?" for _ in _CHUNK_COLUMNS)
            self.db.cursor().executemany(
                f"INSERT OR REPLACE INTO chunks ({', '.join(_CHUNK_COLUMNS)}) VALUES ({marks})", rows
            )
            self.db.commit()
            self.total_chunks += len(with_emb)
            if self.config.auto_save:
                self.save_index()
        self.logger.info(f"Added {len(with_emb)} chunks to storage")

    # --------------------------------------------------------------- search
    def _search_frame(self, config: Optional[SearchConfig], query_embedding=None):
        """Prologue of every search; the caller holds the lock.  ``None``: no index, or an empty one.  Otherwise
        ``(cfg, ntotal, q)``, the query as a ``[1, d]`` float32 array (``None`` when the search has none)."""
        if not self.faiss_index:
            return None
        ntotal = self.faiss_index.ntotal
        if ntotal == 0:
            return None
        # accepts ndarray or a plain list (tests/test_integration.py:203-204 of the reference)
        q = None if query_embedding is None else np.asarray(query_embedding, dtype=np.float32).reshape(1, -1)
        return config or SearchConfig(), ntotal, q

    def _allow_for(self, filters: Optional[Dict[str, Any]], ntotal: int, tombstones_always: bool) -> Optional[np.ndarray]:
        """The allow mask of a search, ``None`` for every row.  Filters are masked only under ``filter_pushdown``.
        Tombstones are masked under ``filter_pushdown`` too (``search``, ``search_range``: the host loop skips them
        otherwise) or, with ``tombstones_always``, in both modes (``search_sessions``, ``search_diverse``: a deleted
        chunk must not stand for its session or repel other picks)."""
        pushdown = bool(self.config.filter_pushdown)
        masked = filters if pushdown and filters else {}
        tombstones = len(self.faiss_id_to_chunk_id) < ntotal
        if masked or (tombstones and (pushdown or tombstones_always)):
            return self._mask_of(masked, ntotal)
        return None

    # ------------------------------------------------- attribute filters (StorageConfig.attribute_filters, filters.py)
    def _sync_attributes(self, ntotal: int) -> None:
        """Bring the index's attribute columns up to date with SQLite, by the rule of ``_sync_session_labels``: only
        the tail ``[synced, ntotal)`` is read and pushed after adds (a timestamp that sorts in front of a stored one
        moves earlier ranks, and that column is pushed whole); everything when the index object was replaced (load,
        restore, ``clear_all_data``, a rebuild) or compacted."""
        if self._attrs.index is not self.faiss_index:
            self._catalog = AttrCatalog()
        lo = self._attrs.rows_of(self.faiss_index)
        if lo >= ntotal:
            return
        chunks: List[Optional[Dict[str, Any]]] = [None] * (ntotal - lo)
        cols = ", ".join(ATTR_COLUMNS)
        for row in self.db.cursor().execute(f"SELECT id, faiss_id, {cols} FROM chunks WHERE faiss_id >= ? AND faiss_id < ?",
                                            (lo, ntotal)):
            if self.faiss_id_to_chunk_id.get(row["faiss_id"]) == row["id"]:
                chunks[row["faiss_id"] - lo] = {c: row[c] for c in ATTR_COLUMNS}
        try:
            first = self._catalog.extend(chunks)
            for col, row0 in first.items():
                self.faiss_index.set_attribute(self._catalog.slot(col), self._catalog.codes[col][row0:ntotal], row0=row0)
        except BaseException:
            # the catalog may be ahead of the columns: forget both, the next sync pushes everything again
            self._attrs, self._catalog = _Synced(), AttrCatalog()
            raise
        self._attrs.rows = ntotal

    def _attribute_path(self) -> bool:
        """Filters go to the GPU: the option is on and the index answers ``where`` with a mask over ALL its rows (the
        sharded facade answers each rank's local part, which no search of the facade takes: it stays on the host loop)."""
        return bool(self.config.attribute_filters) and not self._sharded() and all(
            hasattr(self.faiss_index, m) for m in ("where", "set_attribute"))

    def _live_mask(self, ntotal: int) -> np.ndarray:
        """The rows that hold a live chunk (the tombstone part of ``_allow_mask``), cached under its stamp."""
        stamp = (self._mutations, len(self.faiss_id_to_chunk_id), ntotal, self.total_chunks)
        if self._live_cache is None or self._live_cache[0] != stamp:
            live = np.zeros(ntotal, dtype=bool)
            ids = np.fromiter((fid for fid, cid in self.faiss_id_to_chunk_id.items()
                               if fid < ntotal and self.chunk_id_to_faiss_id.get(cid) == fid), dtype=np.int64)
            live[ids] = True
            self._live_cache = (stamp, live)
        return self._live_cache[1]

    def _mask_of(self, filters: Dict[str, Any], ntotal: int) -> np.ndarray:
        """``_allow_mask(filters, ntotal)``, computed on the GPU where ``attribute_filters`` is on, the index has
        ``where`` and ``compile_filters`` takes the filter; by the host loop otherwise."""
        if self._attribute_path():
            self._sync_attributes(ntotal)
            clauses = compile_filters(filters, self._catalog)
            if clauses is not None:
                live = self._live_mask(ntotal)
                return self.faiss_index.where(clauses, allow=None if bool(live.all()) else live)
        return self._allow_mask(filters, ntotal)

    def _require(self, what: str, *methods: str) -> None:
        """The capability check of a search variant, in front of the lock (no index at all: the search gives ``[]``)."""
        if self.faiss_index and not all(hasattr(self.faiss_index, m) for m in methods):
            raise NotImplementedError(f"{type(self.faiss_index).__name__} has no {what} ({' / '.join(methods)})")

    def _ranked_in_index(self, query_embedding, config: Optional[SearchConfig], filters: Optional[Dict[str, Any]],
                         cap: int, run: Callable) -> List[SearchResult]:
        """The frame of the searches whose ranking runs inside the index (``search_sessions``, ``search_diverse``,
        ``search_recent``, ``search_like``, ``search_hybrid``): tombstones always in the allow mask; ``top_k`` rows are
        fetched, ``max(top_k, max_results)`` where filters are applied on the host, at most ``cap``.
        ``run(q, k, allow, ntotal, cfg)`` is the variant, under the lock: the ``(sims, ids)`` of the one query
        (``[k]`` or ``[1, k]``), to which the post-processing of ``search()`` applies in rank order."""
        with self._lock:
            frame = self._search_frame(config, query_embedding)
            if frame is None or frame[0].top_k <= 0:
                return []
            cfg, ntotal, q = frame
            allow = self._allow_for(filters, ntotal, tombstones_always=True)
            k = cfg.top_k if (self.config.filter_pushdown or not filters) else max(cfg.top_k, cfg.max_results)
            sims, ids = run(q, max(1, min(k, cap)), allow, ntotal, cfg)
            return self._results_in_rank_order(np.ravel(sims).tolist(), np.ravel(ids).tolist(), cfg, filters)

    def search(self, query_embedding, config: Optional[SearchConfig] = None,
               filters: Optional[Dict[str, Any]] = None) -> List[SearchResult]:
        with self._lock:
            frame = self._search_frame(config, query_embedding)
            if frame is None:
                return []
            cfg, ntotal, q = frame
            k = min(cfg.max_results, ntotal, fi.MAX_K)   # (fi.MAX_K = 2048: beyond 128 the index takes passes of 128)
            if k <= 0:
                return []
            allow = self._allow_for(filters, ntotal, tombstones_always=False)
            if allow is not None:
                k = max(1, min(k, cfg.top_k, fi.MAX_K))
            sims, ids = self.faiss_index.search(q, k, normalize=self.config.normalize_embeddings, allow=allow)
            return self._results_in_rank_order(sims[0].tolist(), ids[0].tolist(), cfg, filters)

    _NO_SESSION = object()   # _results_in_rank_order: no session is left out

    def _results_in_rank_order(self, sims, ids, cfg: SearchConfig, filters: Optional[Dict[str, Any]],
                               skip_session: Any = _NO_SESSION, unbounded: bool = False,
                               limit: Optional[int] = None) -> List[SearchResult]:
        """The hits of one query, best first, through the reference's post-processing (``src/storage.py:438-492``):
        threshold, tombstone skip, SQLite row, filters, stop at ``top_k``.  ``skip_session``: chunks of that session
        are left out as well (``search_related``).  ``unbounded`` (``search_range``: the index applied the threshold):
        no threshold here, and the stop is at ``limit`` results, or never."""
        stop = limit if unbounded else cfg.top_k
        out: List[SearchResult] = []
        for score, fid in zip(sims, ids):
            if not unbounded and score < cfg.similarity_threshold:
                continue
            chunk_id = self.faiss_id_to_chunk_id.get(fid)
            if not chunk_id:  # tombstone: row deleted from SQLite, vector still in the index
                continue
            data = self._get_chunk_data(chunk_id)
            if not data:
                continue
            if filters and not self._matches_filters(data, filters):
                continue
            if skip_session is not self._NO_SESSION and data["session_id"] == skip_session:
                continue
            out.append(self._make_result(chunk_id, score, data, cfg))
            if stop is not None and len(out) >= stop:
                break
        return out

    def search_related(self, chunk_id: str, config: Optional[SearchConfig] = None,
                       filters: Optional[Dict[str, Any]] = None, same_session: bool = False) -> List[SearchResult]:
        """Chunks related to a stored chunk -- what the reference's ``related_to`` / ``--related-to`` offers and never
        does (its ``filters["related_to"]`` names no column, so ``_matches_filters`` ignores it; the key stays ignored
        inside ``filters`` here too).  The anchor's STORED row is the query, read where it lies in HBM
        (``IndexFlat.search_by_ids``), and the anchor is never returned.  No second normalisation is applied:
        ``search()`` re-applies ``x / (||x|| + 1e-8)`` to its query, so its scores for the same vector can differ from
        these in the last bits.
        ``same_session=False`` (the reference's default for its ``same_session`` flag) also leaves out every chunk
        whose ``session_id`` equals the anchor's (an anchor without a session has no session mates);
        ``same_session=True`` leaves out the anchor only.  Threshold, tombstones, ``filters``, ``top_k`` and
        ``max_results`` mean what they mean in ``search()``: without ``filter_pushdown`` the best
        ``min(max_results, ntotal - 1, MAX_K - 1)`` rows are fetched and filtered in rank order; with it, filters,
        tombstones and the session rule form the allow mask and ``top_k`` rows are fetched.
        An unknown or deleted ``chunk_id`` raises ``KeyError``; an empty index and one holding only the anchor give ``[]``."""
        with self._lock:
            frame = self._search_frame(config)
            if frame is None:
                return []
            cfg, ntotal, _ = frame
            fid = self.chunk_id_to_faiss_id.get(chunk_id)
            data = self._get_chunk_data(chunk_id) if fid is not None and fid < ntotal else None
            if not data:
                raise KeyError(chunk_id)
            k = min(cfg.max_results, ntotal - 1, fi.MAX_K - 1)
            if k <= 0:
                return []
            session = data["session_id"]
            skip = self._NO_SESSION if same_session or session is None else session
            allow = None
            if self.config.filter_pushdown:
                allow = self._mask_of(filters or {}, ntotal)
                if skip is not self._NO_SESSION:
                    allow = allow.copy()   # (the cached mask stays as it is)
                    mates = self.db.cursor().execute("SELECT faiss_id FROM chunks WHERE session_id = ? AND faiss_id IS NOT NULL",
                                                     (session,)).fetchall()
                    mates = np.array([r[0] for r in mates], dtype=np.int64)
                    allow[mates[mates < ntotal]] = False
                k = max(1, min(k, cfg.top_k))
            sims, ids = self.faiss_index.search_by_ids([fid], k, exclude_self=True, allow=allow)
            return self._results_in_rank_order(sims[0].tolist(), ids[0].tolist(), cfg, filters, skip)

    def _sync_session_labels(self, ntotal: int) -> None:
        """Bring the index's group labels up to date with SQLite: row = ``faiss_id``, label = a dense integer per
        ``session_id`` in order of first appearance; rows without a session (or without a chunk) stay ungrouped
        (``-1``).  Only the tail ``[synced, ntotal)`` is pushed after adds; everything is pushed when the index
        object was replaced (load, restore, ``clear_all_data``, a rebuild into a second index) or compacted."""
        if self._labels.index is not self.faiss_index:
            self._session_labels = {}
        lo = self._labels.rows_of(self.faiss_index)
        if lo >= ntotal:
            return
        labels = np.full(ntotal - lo, -1, dtype=np.int32)
        rows = self.db.cursor().execute(
            "SELECT faiss_id, session_id FROM chunks WHERE faiss_id >= ? AND faiss_id < ? AND session_id IS NOT NULL "
            "ORDER BY faiss_id", (lo, ntotal)).fetchall()
        for fid, session in rows:
            labels[fid - lo] = self._session_labels.setdefault(session, len(self._session_labels))
        self.faiss_index.set_groups(labels, row0=lo)
        self._labels.rows = ntotal

    def search_sessions(self, query_embedding, config: Optional[SearchConfig] = None,
                        filters: Optional[Dict[str, Any]] = None) -> List[SearchResult]:
        """The best chunk of each of the ``top_k`` best SESSIONS, in rank order -- "which conversations are nearest",
        where ``search()`` may return ``top_k`` chunks of one long conversation.  A session is ranked by its best
        chunk; a chunk without a ``session_id`` counts as a session of its own.  The collapse happens inside the index
        (``IndexFlat.search_grouped``: exact, however many chunks one session has), not over an over-fetched list.

        Threshold, tombstones, ``filters`` and ``filter_pushdown`` mean what they mean in ``search()``.  With
        ``filter_pushdown`` the filters form the allow mask, a session is represented by its best MATCHING chunk and
        ``top_k`` groups are fetched.  Without it, ``min(max_results, 128)`` groups are fetched when there are filters
        and groups whose best row fails a filter are dropped on the host, as ``search()`` drops rows: such a session is
        then missing even if another of its chunks matches.  Tombstones are masked out in both modes, so a deleted
        chunk never stands for its session.  An index object without ``search_grouped`` raises
        ``NotImplementedError``."""
        self._require("grouped search", "search_grouped", "set_groups")

        def run(q, k, allow, ntotal, cfg):
            self._sync_session_labels(ntotal)
            sims, ids, _ = self.faiss_index.search_grouped(q, min(k, ntotal), normalize=self.config.normalize_embeddings, allow=allow)
            return sims, ids

        return self._ranked_in_index(query_embedding, config, filters, fi.MAX_GROUP_K, run)

    def search_diverse(self, query_embedding, config: Optional[SearchConfig] = None,
                       filters: Optional[Dict[str, Any]] = None, lam: float = 0.5) -> List[SearchResult]:
        """``top_k`` chunks picked by maximal marginal relevance (``IndexFlat.search_diverse``) -- where ``search()``
        returns the same stack trace or prompt pasted into ten conversations ten times, this returns it once and goes
        on to other passages.  The first result is ``search()``'s first; every further one trades its similarity to
        the query against its similarity to the chunks already chosen (``lam = 1``: ``search()``'s order, ``lam = 0``:
        diversity alone).  Results come in PICK order, each with its ordinary similarity, so they are not sorted by it.
        The pool is the best 32 rows (``4 * k <= 32``) or 128, and the selection runs inside the index over the stored
        rows.

        Threshold, tombstones, ``filters`` and ``filter_pushdown`` mean what they mean in ``search()``; the threshold
        is applied to the picks in pick order.  Tombstones always go into the allow mask, so a deleted chunk neither
        is picked nor repels others.  With ``filter_pushdown`` the filters go there too and ``k = top_k`` picks are
        made.  Without it and with filters, ``k = min(max(top_k, max_results), 128)`` picks are made and filtered in
        pick order, as ``search()`` filters rows: a chunk that fails the filter still stood in the way of its
        near-copies.  An index object without ``search_diverse`` raises ``NotImplementedError``."""
        self._require("diversified search", "search_diverse")

        def run(q, k, allow, ntotal, cfg):
            return self.faiss_index.search_diverse(q, k, lam=lam, normalize=self.config.normalize_embeddings, allow=allow)

        return self._ranked_in_index(query_embedding, config, filters, fi.MAX_DIVERSE_FETCH, run)

    def _row_days(self, lo: int, hi: int) -> np.ndarray:
        """Timestamps of index rows ``[lo, hi)`` in days since the epoch; NaN: no chunk, no or an unparseable timestamp."""
        t = np.full(hi - lo, np.nan, dtype=np.float64)
        rows = self.db.cursor().execute(
            "SELECT faiss_id, timestamp FROM chunks WHERE faiss_id >= ? AND faiss_id < ? AND timestamp IS NOT NULL",
            (lo, hi)).fetchall()
        for fid, ts in rows:
            t[fid - lo] = timestamp_days(ts)
        return t

    def _sync_recency_priors(self, ntotal: int, half_life_days: float, now_days: float) -> float:
        """Bring the index's prior column up to date (``recency_priors`` of the rows' timestamps) and return the
        reference time it is stored against.  The column is never rewritten as time passes: only the tail
        ``[synced, ntotal)`` is pushed after adds.  Everything is pushed when the index object was replaced or
        compacted, when ``half_life_days`` changed, and when the newest timestamp or ``now`` lies more than
        ``RECENCY_MAX_EXPONENT`` half-lives beyond the reference, which then becomes the newest timestamp (a ``now``
        that far beyond the NEWEST row needs no new column: every boost has underflowed, and the weight factor says so)."""
        h = float(half_life_days)
        full = self._priors.index is not self.faiss_index or self._priors_half_life != h or self._priors_t_ref is None
        lo = 0 if full else self._priors.rows
        t = self._row_days(lo, ntotal) if lo < ntotal else np.zeros(0)
        known = t[~np.isnan(t)]
        newest = None if full else self._priors_newest
        if known.size:
            newest = float(known.max()) if newest is None else max(newest, float(known.max()))
        if not full and newest is not None and newest != self._priors_t_ref:
            ref = self._priors_t_ref
            full = (newest - ref) / h > RECENCY_MAX_EXPONENT or (now_days - ref) / h > RECENCY_MAX_EXPONENT
            if full:
                lo, t = 0, self._row_days(0, ntotal)
        if full:
            self._priors.index, self._priors_half_life = self.faiss_index, h
            self._priors_t_ref = newest if newest is not None else now_days
        self._priors_newest = newest
        if lo < ntotal:
            self.faiss_index.set_priors(recency_priors(t, self._priors_t_ref, h), row0=lo)
        self._priors.rows = ntotal
        return self._priors_t_ref

    def search_recent(self, query_embedding, config: Optional[SearchConfig] = None,
                      filters: Optional[Dict[str, Any]] = None, half_life_days: float = 30.0, weight: float = 0.1,
                      now: Optional[datetime] = None) -> List[SearchResult]:
        """``top_k`` chunks ranked by ``similarity + weight * 2^(-age / half_life_days)`` ("prefer the recent ones"; an
        L2 storage ranks by ``distance - weight * 2^(-age / half_life_days)``), ``age`` = ``now`` (default: the
        present) minus the chunk's ``timestamp`` (ISO, naive = UTC; none or unparseable = infinitely old, no boost).
        The ranking runs inside the index over ALL allowed rows (``IndexFlat.search_prior``), not over an over-fetched
        list: a recent chunk is found however far down the plain ranking it sits.  Results come in FUSED order, each
        with its RAW similarity, to which ``similarity_threshold`` applies (as in ``search_diverse``).

        Tombstones always go into the allow mask.  With ``filter_pushdown`` the filters go there too and ``k = top_k``
        rows are fetched; without it and with filters, ``k = min(max(top_k, max_results), 128)`` rows are fetched and
        filtered in rank order.  ``half_life_days <= 0`` or NaN and a ``weight`` that is not finite raise
        ``ValueError``; an index object without ``search_prior`` raises ``NotImplementedError``."""
        h, w = float(half_life_days), float(weight)
        if not (h > 0.0) or not np.isfinite(h):
            raise ValueError(f"search_recent: half_life_days={half_life_days} must be a positive finite number")
        if not np.isfinite(w):
            raise ValueError(f"search_recent: weight={weight} is not finite")
        self._require("prior-weighted search", "search_prior", "set_priors")
        now_days = timestamp_days(now if now is not None else datetime.now(timezone.utc))
        if now_days != now_days:
            raise ValueError(f"search_recent: now={now!r} is not a time")

        def run(q, k, allow, ntotal, cfg):
            t_ref = self._sync_recency_priors(ntotal, h, now_days)
            with np.errstate(over="ignore", under="ignore"):
                w_now = float(np.float32(w * np.exp2(-(now_days - t_ref) / h)))
            _, ids, sims = self.faiss_index.search_prior(q, k, w_now, normalize=self.config.normalize_embeddings, allow=allow)
            return sims, ids

        return self._ranked_in_index(query_embedding, config, filters, fi.MAX_PRIOR_K, run)

    def search_like(self, liked, disliked=(), query_embedding=None, config: Optional[SearchConfig] = None,
                    filters: Optional[Dict[str, Any]] = None, gamma: float = 0.5) -> List[SearchResult]:
        """"More like these chunks, and not like those": ``top_k`` chunks ranked by
        ``best similarity to a liked example - gamma * best similarity to a disliked one`` (an L2 storage: nearest
        liked distance minus ``gamma`` times nearest disliked distance, smaller first).  ``liked`` / ``disliked`` are
        chunk ids -- their STORED rows are the examples, read where they lie in HBM -- and ``query_embedding``, if
        given, is one more positive vector (normalised like the query of ``search()``).  The ranking runs inside the
        index over ALL allowed rows (``IndexFlat.search_examples``), not over an over-fetched list.  Results come in
        FUSED order, each with its RAW best-liked similarity, to which ``similarity_threshold`` applies (as in
        ``search_recent``).  The example chunks are never returned.

        Tombstones always go into the allow mask.  With ``filter_pushdown`` the filters go there too and ``k = top_k``
        rows are fetched; without it and with filters, ``k = min(max(top_k, max_results), 128)`` rows are fetched and
        filtered in rank order.  No positive at all (no liked chunk and no query) raises ``ValueError``, as do more
        than 16 examples and a ``gamma`` that is negative or not finite; an unknown or deleted chunk id raises
        ``KeyError``; an empty index gives ``[]``; an index object without ``search_examples`` raises
        ``NotImplementedError``."""
        liked = [liked] if isinstance(liked, str) else list(liked)
        disliked = [disliked] if isinstance(disliked, str) else list(disliked)
        nvec = 0 if query_embedding is None else 1
        _, g = fi.example_args(1, gamma, len(liked) + nvec, len(liked) + len(disliked) + nvec, "search_like")
        self._require("search by examples", "search_examples")

        def run(q, k, allow, ntotal, cfg):
            fids = []
            for chunk_id in liked + disliked:
                fid = self.chunk_id_to_faiss_id.get(chunk_id)
                if fid is None or fid >= ntotal or not self._get_chunk_data(chunk_id):
                    raise KeyError(chunk_id)
                fids.append(fid)
            _, ids, sims = self.faiss_index.search_examples(
                pos=q, pos_ids=fids[:len(liked)], neg_ids=fids[len(liked):], k=k, gamma=g,
                normalize=self.config.normalize_embeddings, exclude_ids=True, allow=allow)
            return sims, ids

        return self._ranked_in_index(query_embedding, config, filters, fi.MAX_EXAMPLES_K, run)

    def topics(self, n_topics: int = 20, filters: Optional[Dict[str, Any]] = None, niter: int = 20, seed: int = 0,
               examples: int = 3) -> List[Topic]:
        """"What is in here": a k-means of the live chunks that match ``filters`` into ``n_topics`` clusters on the GPU
        (``IndexFlat.kmeans``), each named by the ``examples`` chunks nearest its centroid.  Tombstones are always left
        out; ``n_topics`` is cut to the number of live matching chunks (one chunk: one topic, no clustering).  One
        ``kmeans`` and one ``search(centroids, examples)`` under the same mask.  Largest topic first.  An empty index
        gives ``[]``; an index object without ``kmeans`` raises ``NotImplementedError``."""
        if n_topics < 1 or examples < 1:
            raise ValueError(f"topics: n_topics={n_topics} and examples={examples} must be positive")
        with self._lock:
            frame = self._search_frame(SearchConfig())
            if frame is None:
                return []
            cfg, ntotal, _ = frame
            if not hasattr(self.faiss_index, "kmeans"):
                raise NotImplementedError(f"{type(self.faiss_index).__name__} has no k-means (kmeans)")
            allow = self._mask_of(filters or {}, ntotal)
            live = int(allow.sum())
            nc = min(int(n_topics), live, fi.MAX_CENTROIDS)
            if nc == 0:
                return []
            if nc == 1:   # (k-means needs two centroids: the one topic is everything, named by the mean's neighbours)
                rows = np.flatnonzero(allow)
                cent = self.faiss_index.reconstruct_batch(rows[: 1 << 16]).astype(np.float64).mean(axis=0, keepdims=True)
                if self.config.normalize_embeddings:
                    cent /= max(float(np.linalg.norm(cent)), 1e-30)
                cent = cent.astype(np.float32)
                assign = np.where(allow, 0, -1)
            else:
                res = self.faiss_index.kmeans(nc, niter=niter, seed=seed, allow=allow)
                cent, assign = res.centroids, np.asarray(res.assign)
            k = max(1, min(int(examples), live, fi.MAX_K))
            sims, ids = self.faiss_index.search(cent, k, normalize=False, allow=allow)
            out: List[Topic] = []
            for c in range(nc):
                members = np.flatnonzero(assign == c)
                if members.size == 0:
                    continue
                near = self._results_in_rank_order(sims[c].tolist(), ids[c].tolist(), cfg, None, unbounded=True, limit=k)
                if not near:
                    continue
                chunk_ids = [self.faiss_id_to_chunk_id[int(f)] for f in members if int(f) in self.faiss_id_to_chunk_id]
                out.append(Topic(size=int(members.size), representative=near[0], examples=near, chunk_ids=chunk_ids))
            out.sort(key=lambda t: -t.size)   # (stable: equal sizes stay in centroid order)
            return out

    def map(self, filters: Optional[Dict[str, Any]] = None, n_topics: int = 0, seed: int = 0,
            niter: int = 20) -> List[MapPoint]:
        """A 2-D map of the live chunks that match ``filters``: each chunk at its coordinates on the first two principal
        components of the selection, computed on the GPU (one ``IndexFlat.pca(2, allow=mask)``, then ``transform`` over
        the rows in ranges of at most 2^20, of which the allowed rows are kept).  Tombstones are always left out.
        ``n_topics >= 2`` adds as ``topic`` the ``kmeans`` assignment under the same mask, ``seed`` and ``niter``: the
        clusters of ``topics`` called with the same ``n_topics``, ``filters``, ``seed`` and ``niter``; else ``topic`` is
        ``None``.  An empty selection gives ``[]``; a single chunk lies at ``(0, 0)``; an
        index object without ``pca`` raises ``NotImplementedError``."""
        with self._lock:
            frame = self._search_frame(SearchConfig())
            if frame is None:
                return []
            _, ntotal, _ = frame
            if not (hasattr(self.faiss_index, "pca") and hasattr(self.faiss_index, "transform")):
                raise NotImplementedError(f"{type(self.faiss_index).__name__} has no PCA (pca / transform)")
            allow = self._mask_of(filters or {}, ntotal)
            rows = np.flatnonzero(allow)
            if rows.size == 0:
                return []
            topic = None
            if n_topics >= 2:
                nc = min(int(n_topics), int(rows.size), fi.MAX_CENTROIDS)
                if nc >= 2:
                    topic = np.asarray(self.faiss_index.kmeans(nc, niter=niter, seed=seed, allow=allow).assign)[rows]
                else:
                    topic = np.zeros(rows.size, dtype=np.int64)
            xy = np.zeros((rows.size, 2), dtype=np.float32)
            if rows.size > 1:
                res = self.faiss_index.pca(2, allow=allow)
                b = fi.pca_offset(res.components, res.mean)
                step = 1 << 20
                for lo in range(0, ntotal, step):
                    n = min(step, ntotal - lo)
                    keep = allow[lo:lo + n]
                    if keep.any():
                        at = np.searchsorted(rows, lo)
                        part = self.faiss_index.transform(res.components, b, lo, n)[keep]
                        xy[at:at + part.shape[0]] = part
            out: List[MapPoint] = []
            for j, f in enumerate(rows.tolist()):
                cid = self.faiss_id_to_chunk_id.get(f)
                if cid is not None:
                    out.append(MapPoint(cid, float(xy[j, 0]), float(xy[j, 1]), None if topic is None else int(topic[j])))
            return out

    def _sync_terms(self, ntotal: int) -> None:
        """Bring the index's term lists up to date with SQLite: row = ``faiss_id``, list = ``lexical.terms_of`` of the
        chunk's stored text; a row without a live chunk gets the empty list.  Only the tail ``[synced, ntotal)`` is
        pushed after adds (the lists are append-only in row order); everything is pushed again when the index object
        was replaced or compacted, by the rule of ``_sync_session_labels``."""
        from .lexical import terms_of

        lo = self._terms.rows_of(self.faiss_index)
        if lo >= ntotal:
            return
        lists: List[List[int]] = [[] for _ in range(ntotal - lo)]
        rows = self.db.cursor().execute("SELECT faiss_id, text FROM chunks WHERE faiss_id >= ? AND faiss_id < ?",
                                        (lo, ntotal)).fetchall()
        for fid, text in rows:
            lists[fid - lo] = terms_of(text)
        self.faiss_index.set_terms(lists, row0=lo)
        self._terms.rows = ntotal

    def keywords(self, chunk_ids: Optional[List[str]] = None, filters: Optional[Dict[str, Any]] = None, n: int = 10,
                 min_count: int = 2) -> List[Keyword]:
        """"Which words set these chunks apart": the ``n`` terms most over-represented in a selection of chunks against
        all live chunks, counted and ranked on the GPU (``IndexFlat.significant_terms``, JLH score; Elasticsearch's
        ``significant_terms``).  The selection is the live chunks that match ``filters`` and, where given, are named by
        ``chunk_ids`` (unknown and deleted ids are ignored) -- ``keywords(chunk_ids=topic.chunk_ids)`` names a topic,
        ``keywords(chunk_ids=[r.chunk_id for r in hits])`` says why these hits.  A word counts once per chunk and must
        be in at least ``min_count`` selected chunks.  Each ``Keyword`` carries the word as it first appears (after BERT's
        word splitting) in the selected chunks' stored text in ``faiss_id`` order, its term id, the chunks of the
        selection and of the background that hold it, and the score; best first.  An empty selection gives ``[]``; an
        index object without ``significant_terms`` raises ``NotImplementedError``."""
        from .lexical import significant_args, words_of_terms

        n, min_count = significant_args(n, min_count, "keywords")
        self._require("significant terms", "significant_terms", "set_terms")
        with self._lock:
            frame = self._search_frame(SearchConfig())
            if frame is None:
                return []
            _, ntotal, _ = frame
            self._sync_terms(ntotal)
            live = self._mask_of({}, ntotal)
            sel = self._mask_of(filters or {}, ntotal)
            if chunk_ids is not None:
                named = np.zeros(ntotal, dtype=bool)
                for cid in chunk_ids:
                    fid = self.chunk_id_to_faiss_id.get(cid)
                    if fid is not None and fid < ntotal:
                        named[fid] = True
                sel = sel & named
            rows = np.flatnonzero(sel)
            if rows.size == 0:
                return []
            res = self.faiss_index.significant_terms(allow=sel, m=n, min_count=min_count, background=live)
            if len(res.terms) == 0:
                return []
            cur = self.db.cursor().execute(
                "SELECT faiss_id, id, text FROM chunks WHERE faiss_id >= ? AND faiss_id <= ? ORDER BY faiss_id",
                (int(rows[0]), int(rows[-1])))
            texts = (text for fid, cid, text in cur if sel[fid] and self.faiss_id_to_chunk_id.get(fid) == cid)
            words = words_of_terms(texts, res.terms)
            return [Keyword(words.get(int(t), ""), int(t), int(f), int(b), float(s))
                    for t, f, b, s in zip(res.terms, res.fg, res.bg, res.score)]

    def search_hybrid(self, query_text: str, query_embedding, config: Optional[SearchConfig] = None,
                      filters: Optional[Dict[str, Any]] = None, alpha: float = 0.3, k1: float = 1.2,
                      b: float = 0.75) -> List[SearchResult]:
        """``top_k`` chunks ranked by ``similarity + alpha * lex`` (an L2 storage: ``distance - alpha * lex``), ``lex`` =
        the BM25 score of the words of ``query_text`` against the chunk's stored text, normalised to ``[0, 1)`` by the
        largest value the query can reach -- the keyword side a sentence encoder blurs: identifiers, error codes, flag
        and file names.  The ranking runs inside the index over ALL allowed rows (``IndexFlat.search_hybrid``), not
        over an over-fetched dense list: a chunk that holds a rare query word is found however far down the plain
        ranking it sits.  Results come in FUSED order, each with its RAW similarity, to which
        ``similarity_threshold`` applies (as in ``search_recent``).

        Query terms are the distinct ``lexical.terms_of(query_text)`` in first-occurrence order; terms no chunk holds
        are dropped, and beyond 32 terms the 32 rarest are kept (still in first-occurrence order).  Weights are
        ``lexical.bm25_weights(..., normalized=True)``.  Without a usable term the ranking is that of ``search()``.
        Words are matched whole after BERT's word splitting: no stemming, no stop list (the idf handles the latter).

        Tombstones always go into the allow mask.  With ``filter_pushdown`` the filters go there too and ``k = top_k``
        rows are fetched; without it and with filters, ``k = min(max(top_k, max_results), 128)`` rows are fetched and
        filtered in rank order.  ``alpha = 0.3`` is a default NOBODY HAS TUNED: there is no relevance data offline.
        An ``alpha``, ``k1`` or ``b`` the index would refuse raises ``ValueError``; an index object without
        ``search_hybrid`` raises ``NotImplementedError``."""
        from .lexical import bm25_weights, terms_of

        a = float(alpha)
        if not np.isfinite(a):
            raise ValueError(f"search_hybrid: alpha={alpha} is not finite")
        self._require("hybrid search", "search_hybrid", "set_terms", "term_stats")

        def run(q, k, allow, ntotal, cfg):
            self._sync_terms(ntotal)
            terms = list(dict.fromkeys(terms_of(query_text)))
            weights = np.zeros(0, np.float32)
            if terms:
                df, ndocs, _ = self.faiss_index.term_stats(terms)
                known = [j for j in range(len(terms)) if df[j] > 0]
                if len(known) > fi.MAX_QUERY_TERMS:   # the rarest, still in first-occurrence order
                    known = sorted(sorted(known, key=lambda j: (int(df[j]), j))[:fi.MAX_QUERY_TERMS])
                terms = [terms[j] for j in known]
                weights = bm25_weights(np.asarray(df)[known], ndocs, k1=k1, normalized=True)
            _, ids, sims, _ = self.faiss_index.search_hybrid(q, terms, weights, k, a, k1=k1, b=b,
                                                             normalize=self.config.normalize_embeddings, allow=allow)
            return sims, ids

        return self._ranked_in_index(query_embedding, config, filters, fi.MAX_HYBRID_K, run)

    # ------------------------------------------------------- sparse vectors
    @property
    def sparse_path(self) -> Path:
        """The file beside the index file that holds the chunks' sparse vectors."""
        return Path(str(self.index_path) + ".sparse.npz")

    @staticmethod
    def _sparse_model_name(sparse_encoder) -> str:
        name = getattr(sparse_encoder, "model_name", None) or getattr(sparse_encoder, "model_dir", None)
        return str(name) if name else type(sparse_encoder).__name__

    def _drop_sparse_file(self) -> None:
        self._sparse_saved = None
        if self.sparse_path.exists():
            self.sparse_path.unlink()

    def _save_sparse(self, ntotal: int) -> None:
        """``save_index``'s second file: ``offsets``, ``terms``, ``weights`` of all ``ntotal`` rows, the rows that have a
        vector and the model's name, as one ``.npz``, written whole through a temporary sibling.  Skipped while the
        file already says the same; nothing is written for an index that carries no vectors."""
        ix = self.faiss_index
        rows = self._sparse.rows if self._sparse.index is ix else 0
        if rows <= 0 or not hasattr(ix, "get_sparse"):
            return
        state = (self._sparse_model, rows, ntotal)
        if state == self._sparse_saved and self.sparse_path.exists():
            return
        off, terms, weights = ix.get_sparse(0, ntotal)
        tmp = str(self.sparse_path) + ".tmp.npz"
        np.savez(tmp, offsets=off, terms=terms, weights=weights, rows=np.int64(rows), model=np.array(self._sparse_model or ""))
        os.replace(tmp, str(self.sparse_path))
        _fsync_dir(self.sparse_path.parent)
        self._sparse_saved = state

    def _load_sparse(self) -> None:
        """The vectors of ``_save_sparse`` back into a freshly loaded index, when the file is there and speaks of as many
        rows as the index has; otherwise nothing, and ``index_sparse`` encodes lazily."""
        ix = self.faiss_index
        if not self.sparse_path.exists() or not hasattr(ix, "set_sparse"):
            return
        try:
            with np.load(str(self.sparse_path)) as z:
                off, terms, weights = z["offsets"], z["terms"], z["weights"]
                rows, model = int(z["rows"]), str(z["model"])
            if off.shape[0] - 1 != ix.ntotal or not 0 < rows <= ix.ntotal:
                self.logger.warning(f"{self.sparse_path.name} speaks of {off.shape[0] - 1} rows, the index has {ix.ntotal}: ignored")
                return
            e = int(off[rows])
            ix.set_sparse((np.ascontiguousarray(off[:rows + 1]), terms[:e], weights[:e]), row0=0)
        except Exception as e:  # a corrupt or foreign file: the lazy sync encodes again
            self.logger.warning(f"Could not load the sparse vectors: {e}")
            return
        self._sparse.index, self._sparse.rows = ix, rows
        self._sparse_model = model or None
        self._sparse_saved = (self._sparse_model, rows, ix.ntotal)
        self.logger.info(f"Loaded the sparse vectors of {rows} rows")

    def _sync_sparse(self, ntotal: int, sparse_encoder, batch_size: int = 32) -> int:
        """Bring the index's sparse vectors up to date with SQLite, in the shape of ``_sync_terms``: row = ``faiss_id``,
        vector = ``sparse_encoder.encode_documents`` of the chunk's stored text; a row without a live chunk gets the
        empty vector.  Only the tail ``[synced, ntotal)`` is encoded after adds; everything again when the index
        object was replaced or the vectors came from another model.  Returns the number of texts encoded."""
        name = self._sparse_model_name(sparse_encoder)
        lo = self._sparse.rows_of(self.faiss_index)
        if lo > 0 and self._sparse_model != name:
            lo = 0
        if lo >= ntotal:
            return 0
        rows = self.db.cursor().execute("SELECT faiss_id, text FROM chunks WHERE faiss_id >= ? AND faiss_id < ? ORDER BY faiss_id",
                                        (lo, ntotal)).fetchall()
        rows = [(fid, text) for fid, text in rows if self.faiss_id_to_chunk_id.get(fid) is not None]
        empty = (np.zeros(0, np.int64), np.zeros(0, np.float32))
        vectors = [empty] * (ntotal - lo)
        if rows:
            encoded = sparse_encoder.encode_documents([text or "" for _, text in rows], batch_size=batch_size)
            for (fid, _), v in zip(rows, encoded):
                t, w = np.asarray(v[0], np.int64), np.asarray(v[1], np.float32)
                keep = w > 0.0                   # (a zero weight means "not in the vector")
                vectors[fid - lo] = (t[keep], w[keep])
        self.faiss_index.set_sparse(vectors, row0=lo)
        self._sparse.rows, self._sparse_model = ntotal, name
        return len(rows)

    def index_sparse(self, sparse_encoder, batch_size: int = 32) -> int:
        """Give every live chunk that has none yet a learned sparse vector (``SparseEncoder.encode_documents`` of its
        stored text, stored in the index by ``IndexFlat.set_sparse``); tombstones get the empty vector.  Lazy: only
        rows added since the last call are encoded, and ``search_sparse`` / ``search_hybrid_sparse`` call it
        themselves.  ``save_index`` writes the vectors beside the index file and ``initialize`` loads them again, so a
        corpus is not encoded on every load.  Returns the number of texts encoded."""
        self._require("sparse vectors", "set_sparse", "search_sparse")
        with self._lock:
            frame = self._search_frame(SearchConfig())
            if frame is None:
                return 0
            done = self._sync_sparse(frame[1], sparse_encoder, batch_size)
            if done and self.config.auto_save:
                self._save_sparse(frame[1])
            return done

    def _sparse_query(self, query_text: str, sparse_encoder):
        v = sparse_encoder.encode_queries([query_text or ""], max_terms=fi.MAX_SPARSE_QUERY_TERMS)[0]
        t, w = np.asarray(v[0], np.int64), np.asarray(v[1], np.float32)
        keep = w != 0.0
        return t[keep], w[keep]

    def search_sparse(self, query_text: str, sparse_encoder, config: Optional[SearchConfig] = None,
                      filters: Optional[Dict[str, Any]] = None) -> List[SearchResult]:
        """Learned sparse retrieval as a FIRST stage: ``top_k`` chunks ranked by the dot product of the query's sparse
        vector (``sparse_encoder.encode_queries``, at most 64 terms) with the chunks' sparse vectors, over ALL allowed
        rows inside the index (``IndexFlat.search_sparse``); no dense row is read and no query embedding is needed.
        Only chunks that share a term with the query are returned.  Each result's ``similarity`` is the dot product,
        to which ``similarity_threshold`` applies.  Tombstones and filters as in ``search_hybrid``."""
        self._require("sparse search", "set_sparse", "search_sparse")

        def run(q, k, allow, ntotal, cfg):
            self._sync_sparse(ntotal, sparse_encoder)
            t, w = self._sparse_query(query_text, sparse_encoder)
            sims, ids = self.faiss_index.search_sparse(t, w, k, allow=allow)
            return sims, ids

        return self._ranked_in_index(None, config, filters, fi.MAX_HYBRID_K, run)

    def search_hybrid_sparse(self, query_text: str, query_embedding, sparse_encoder, alpha: float = 0.3,
                             config: Optional[SearchConfig] = None,
                             filters: Optional[Dict[str, Any]] = None) -> List[SearchResult]:
        """``search_hybrid`` with the learned sparse dot product in the place of BM25: ``top_k`` chunks ranked by
        ``similarity + alpha * sp`` (an L2 storage: ``distance - alpha * sp``) over ALL allowed rows inside the index
        (``IndexFlat.search_hybrid_sparse``).  Results come in FUSED order, each with its RAW similarity, to which
        ``similarity_threshold`` applies.  ``sp`` is not normalised: it grows with the number and weight of the shared
        terms.  ``alpha = 0.3`` is a default NOBODY HAS TUNED, as it is for BM25: there is no relevance data offline."""
        a = float(alpha)
        if not np.isfinite(a):
            raise ValueError(f"search_hybrid_sparse: alpha={alpha} is not finite")
        self._require("sparse hybrid search", "set_sparse", "search_hybrid_sparse")

        def run(q, k, allow, ntotal, cfg):
            self._sync_sparse(ntotal, sparse_encoder)
            t, w = self._sparse_query(query_text, sparse_encoder)
            _, ids, sims, _ = self.faiss_index.search_hybrid_sparse(q, t, w, k, a, normalize=self.config.normalize_embeddings,
                                                                    allow=allow)
            return sims, ids

        return self._ranked_in_index(query_embedding, config, filters, fi.MAX_HYBRID_K, run)

    # ------------------------------------------------------- token matrices (late interaction)
    @property
    def tokens_path(self) -> Path:
        """The file beside the index file that holds the chunks' token matrices."""
        return Path(str(self.index_path) + ".tokens.npz")

    def _drop_tokens_file(self) -> None:
        self._tokens_saved = None
        if self.tokens_path.exists():
            self.tokens_path.unlink()

    def _save_tokens(self, ntotal: int) -> None:
        """``save_index``'s third file, in the shape of ``_save_sparse``: ``offsets``, the uint16 ``tokens``, ``P``, the
        rows that have a matrix and the model's name, as one ``.npz``, written whole through a temporary sibling.
        Skipped while the file already says the same; nothing is written for an index that carries no matrices."""
        ix = self.faiss_index
        rows = self._tokens.rows if self._tokens.index is ix else 0
        if rows <= 0 or not hasattr(ix, "get_tokens"):
            return
        state = (self._tokens_model, rows, ntotal)
        if state == self._tokens_saved and self.tokens_path.exists():
            return
        tmp = str(self.tokens_path) + ".tmp.npz"
        codec = ix.get_token_codec() if getattr(ix, "token_codec_bits", 0) else None
        if codec is not None:   # the COMPRESSED form: codec and canonical codes, never the decoded matrices
            off, codes, res = ix.get_token_codes(0, ntotal)
            np.savez(tmp, offsets=off, codes=codes, res=res, P=np.int64(codec.P), rows=np.int64(rows),
                     model=np.array(self._tokens_model or ""), nbits=np.int64(codec.nbits),
                     centroids=(np.ascontiguousarray(codec.centroids).view(np.uint32) >> 16).astype(np.uint16),
                     cutoffs=codec.cutoffs, weights=codec.weights)
        else:
            off, tok = ix.get_tokens(0, ntotal)
            np.savez(tmp, offsets=off, tokens=tok, P=np.int64(tok.shape[1]), rows=np.int64(rows), model=np.array(self._tokens_model or ""))
        os.replace(tmp, str(self.tokens_path))
        _fsync_dir(self.tokens_path.parent)
        self._tokens_saved = state

    def _load_tokens(self) -> None:
        """The matrices of ``_save_tokens`` back into a freshly loaded index, when the file is there and speaks of as
        many rows as the index has; otherwise nothing, and ``index_tokens`` encodes lazily."""
        ix = self.faiss_index
        if not self.tokens_path.exists() or not hasattr(ix, "set_tokens"):
            return
        try:
            with np.load(str(self.tokens_path)) as z:
                compressed = "codes" in z.files
                off = z["offsets"]
                P, rows, model = int(z["P"]), int(z["rows"]), str(z["model"])
                if compressed:
                    codes, res = z["codes"], z["res"]
                    codec = fi.TokenCodec((z["centroids"].astype(np.uint32) << 16).view(np.float32), int(z["nbits"]),
                                          z["cutoffs"], z["weights"])
                else:
                    tok = z["tokens"]
            if off.shape[0] - 1 != ix.ntotal or not 0 < rows <= ix.ntotal:
                self.logger.warning(f"{self.tokens_path.name} speaks of {off.shape[0] - 1} rows, the index has {ix.ntotal}: ignored")
                return
            if compressed:
                ix.set_token_codec(codec)
                ix.set_token_codes(np.ascontiguousarray(off[:rows + 1]), codes[:int(off[rows])], res[:int(off[rows])], row0=0)
                self._tokens_codec_model = model or None
            else:   # a file of the uncompressed shape: into an index without a codec
                ix.set_tokens((np.ascontiguousarray(off[:rows + 1]), tok[:int(off[rows])], P), row0=0)
        except Exception as e:  # a corrupt or foreign file: the lazy sync encodes again
            self.logger.warning(f"Could not load the token matrices: {e}")
            return
        self._tokens.index, self._tokens.rows = ix, rows
        self._tokens_model = model or None
        self._tokens_saved = (self._tokens_model, rows, ix.ntotal)
        self.logger.info(f"Loaded the token matrices of {rows} rows")

    def _sync_tokens(self, ntotal: int, late, batch_size: int = 32) -> int:
        """Bring the index's token matrices up to date with SQLite, in the shape of ``_sync_sparse``: row =
        ``faiss_id``, matrix = ``late.encode_documents`` of the chunk's stored text with the skiplist's tokens dropped;
        a row without a live chunk gets the empty matrix.  Only the tail ``[synced, ntotal)`` is encoded after adds;
        everything again when the index object was replaced or the matrices came from another model.  Returns the
        number of texts encoded."""
        P = int(late.token_dim)
        if P % 32 or not 32 <= P <= 128:
            raise ValueError(f"index_tokens: the model's token vectors have P={P}; the index stores a multiple of 32 in "
                             "[32, 128] (a checkpoint with a token projection)")
        name = self._sparse_model_name(late)
        lo = self._tokens.rows_of(self.faiss_index)
        if lo > 0 and self._tokens_model != name:
            lo = 0
        if lo >= ntotal:
            return 0
        rows = self.db.cursor().execute("SELECT faiss_id, text FROM chunks WHERE faiss_id >= ? AND faiss_id < ? ORDER BY faiss_id",
                                        (lo, ntotal)).fetchall()
        rows = [(fid, text) for fid, text in rows if self.faiss_id_to_chunk_id.get(fid) is not None]
        mats: List[Any] = [np.zeros((0, P), np.uint16)] * (ntotal - lo)
        keep: List[Any] = [None] * (ntotal - lo)
        if rows:
            encoded, flags = late.encode_documents([text or "" for _, text in rows], batch_size=batch_size)
            for n, (fid, _) in enumerate(rows):
                mats[fid - lo] = encoded[n]
                keep[fid - lo] = flags[n] if flags is not None else None
        if lo == 0:
            self._token_codec_for(mats, keep, name)
        self.faiss_index.set_tokens(mats, keep=keep, row0=lo)
        self._tokens.rows, self._tokens_model = ntotal, name
        return len(rows)

    def _token_codec_for(self, mats, keep, name: Optional[str]) -> None:
        """Before the matrices are written from row 0: give the index the token codec that
        ``StorageConfig.token_codec_bits`` asks for -- trained on this first batch of encoded chunks
        (``train_token_codec``), once per index and model -- or take a codec away that the configuration no longer asks
        for.  Fewer than 16 tokens train nothing: they are stored as they are."""
        ix = self.faiss_index
        bits = int(self.config.token_codec_bits)
        have = int(getattr(ix, "token_codec_bits", 0))
        if bits == 0 and have == 0:
            return
        if bits and not hasattr(ix, "set_token_codec"):
            raise NotImplementedError("token_codec_bits needs an index with set_token_codec")
        if bits and have == bits and self._tokens_codec_model == name:
            return
        off, tok, _ = fi.tokens_as_csr(mats, keep, what="index_tokens")
        ix.drop_tokens()
        if bits == 0 or tok.shape[0] < 16:
            ix.set_token_codec(None)
            self._tokens_codec_model = None
            return
        nc = int(min(max(int(self.config.token_codec_centroids), 2), 4096, tok.shape[0] // 8))
        ix.set_token_codec(fi.train_token_codec((off, tok, tok.shape[1]), nc, nbits=bits, device=int(self.config.device)))
        self._tokens_codec_model = name
        self.logger.info(f"Trained a token codec: {nc} centroids, {bits} bits, on {tok.shape[0]} tokens")

    def index_tokens(self, late, batch_size: int = 32) -> int:
        """Give every live chunk that has none yet a token matrix (``LateInteraction.encode_documents`` of its stored
        text, kept tokens only, stored in the index by ``IndexFlat.set_tokens``); tombstones get the empty matrix.
        Lazy: only rows added since the last call are encoded, and ``search_late`` / ``search_late_reranked`` call it
        themselves.  ``save_index`` writes the matrices beside the index file and ``initialize`` loads them again, so a
        corpus is not encoded on every load.  Returns the number of texts encoded."""
        self._require("token matrices", "set_tokens", "search_maxsim")
        with self._lock:
            frame = self._search_frame(SearchConfig())
            if frame is None:
                return 0
            done = self._sync_tokens(frame[1], late, batch_size)
            if done and self.config.auto_save:
                self._save_tokens(frame[1])
            return done

    def search_late(self, query_text: str, late, config: Optional[SearchConfig] = None,
                    filters: Optional[Dict[str, Any]] = None) -> List[SearchResult]:
        """Late interaction as a FIRST stage: ``top_k`` chunks ranked by MaxSim of the query's token matrix
        (``late.encode_queries``) with the chunks' stored matrices, over ALL allowed rows inside the index
        (``IndexFlat.search_maxsim``); no dense row is read, no query embedding is needed and no text goes through the
        encoder again.  Each result's ``similarity`` is the MaxSim score, to which ``similarity_threshold`` applies.
        Tombstones and filters as in ``search_sparse``.  With ``StorageConfig.late_candidates > 0`` on an index with a
        token codec only that many chunks, chosen by the MaxSim of their tokens' centroids, are scored exactly
        (``IndexFlat.search_maxsim_pruned``): the scores returned are still exact, a chunk outside the candidates is
        not seen."""
        self._require("late-interaction search", "set_tokens", "search_maxsim")

        def run(q, k, allow, ntotal, cfg):
            self._sync_tokens(ntotal, late)
            q_mat = late.encode_queries([query_text or ""])[0][0]
            ncand = int(self.config.late_candidates)
            if ncand > 0 and getattr(self.faiss_index, "token_codec_bits", 0) and hasattr(self.faiss_index, "search_maxsim_pruned"):
                return self.faiss_index.search_maxsim_pruned(q_mat, k, min(max(ncand, k), fi.MAX_MAXSIM_ROWS), allow=allow)
            return self.faiss_index.search_maxsim(q_mat, k, allow=allow)

        return self._ranked_in_index(None, config, filters, fi.MAX_HYBRID_K, run)

    def search_late_many(self, query_texts: Sequence[str], late, config: Optional[SearchConfig] = None,
                         filters: Optional[Dict[str, Any]] = None) -> List[List[SearchResult]]:
        """``search_late`` for several queries at once: element ``i`` equals ``search_late(query_texts[i], late, config,
        filters)`` in ids and score bits.  One ``late.encode_queries`` call (each query in a forward pass of its own, as
        ``search_late`` encodes it), ONE allow mask and one ``IndexFlat.search_maxsim_batch`` -- the
        token store is read once per group of queries, not once per query.  Where ``search_late`` goes through
        ``search_maxsim_pruned`` (``late_candidates > 0`` on an index with a token codec) the candidate sets differ per
        query and nothing is shared: the queries then run as single pruned calls."""
        self._require("late-interaction search", "set_tokens", "search_maxsim", "search_maxsim_batch")
        texts = [t or "" for t in query_texts]
        if not texts:
            return []
        with self._lock:
            frame = self._search_frame(config)
            if frame is None or frame[0].top_k <= 0:
                return [[] for _ in texts]
            cfg, ntotal, _ = frame
            allow = self._allow_for(filters, ntotal, tombstones_always=True)
            k = cfg.top_k if (self.config.filter_pushdown or not filters) else max(cfg.top_k, cfg.max_results)
            k = max(1, min(k, fi.MAX_HYBRID_K))
            self._sync_tokens(ntotal, late)
            # (one query per forward pass: the encoder picks its tiling by the tokens of a batch, so a query encoded
            # beside others can differ in the last bits of its bf16 tokens from the matrix search_late forms for it)
            q_mats = late.encode_queries(texts, batch_size=1)[0]
            ncand = int(self.config.late_candidates)
            if ncand > 0 and getattr(self.faiss_index, "token_codec_bits", 0) and hasattr(self.faiss_index, "search_maxsim_pruned"):
                pairs = [self.faiss_index.search_maxsim_pruned(q, k, min(max(ncand, k), fi.MAX_MAXSIM_ROWS), allow=allow)
                         for q in q_mats]
                sims, ids = np.concatenate([p[0] for p in pairs]), np.concatenate([p[1] for p in pairs])
            else:
                sims, ids = [], []
                for b0 in range(0, len(q_mats), fi.MAX_MAXSIM_QUERIES):
                    d, i = self.faiss_index.search_maxsim_batch(q_mats[b0:b0 + fi.MAX_MAXSIM_QUERIES], k, allow=allow)
                    sims.append(d)
                    ids.append(i)
                sims, ids = np.concatenate(sims), np.concatenate(ids)
            return [self._results_in_rank_order(sims[b].tolist(), ids[b].tolist(), cfg, filters) for b in range(len(texts))]

    def search_reranked(self, query_text: str, query_embedding, reranker, config: Optional[SearchConfig] = None,
                        filters: Optional[Dict[str, Any]] = None, fetch: int = 50) -> List[Reranked]:
        """Retrieve, then re-read: the ordinary ``search`` for ``max(fetch, top_k)`` hits, each ``(query_text, chunk
        text)`` pair scored by ``reranker.predict`` (a ``CrossEncoder``: one forward pass over ``[CLS] query [SEP] text
        [SEP]`` per hit), and the ``top_k`` best by that score, best first; ties keep the plain search's order.  Each
        ``Reranked`` carries the plain ``SearchResult`` (its bi-encoder ``similarity`` untouched), the reranker's
        ``score`` and ``rank_before``, the hit's position in the plain ranking.  Tombstones, filters and
        ``similarity_threshold`` behave as in ``search``; the reranker's hidden size need not match the index.  A chunk
        the plain search ranks below ``fetch`` is never seen: re-ranking reorders, it does not retrieve.
        ``reranker`` is any object with ``predict(pairs)``: a ``LateInteraction`` serves as well (the query is encoded
        once, every hit gets one text-only forward pass and a MaxSim score)."""
        cfg = config or SearchConfig()
        if cfg.top_k <= 0:
            return []
        n = max(int(fetch), cfg.top_k)
        wide = SearchConfig(top_k=n, similarity_threshold=cfg.similarity_threshold, include_metadata=cfg.include_metadata,
                            include_text=True, max_results=max(cfg.max_results, n))
        hits = self.search(query_embedding, wide, filters)
        if not hits:
            return []
        scores = np.asarray(reranker.predict([(query_text, h.text or "") for h in hits]), dtype=np.float32).reshape(-1)
        if scores.size != len(hits):
            raise ValueError(f"search_reranked: the reranker returned {scores.size} scores for {len(hits)} pairs")
        out = []
        for i in np.argsort(-scores, kind="stable")[:cfg.top_k]:
            h = hits[int(i)]
            if not cfg.include_text:
                h.text, h.chunk = None, None
            out.append(Reranked(h, float(scores[i]), int(i)))
        return out

    def search_late_reranked(self, query_text: str, query_embedding, late, config: Optional[SearchConfig] = None,
                             filters: Optional[Dict[str, Any]] = None, fetch: int = 50) -> List[Reranked]:
        """``search_reranked(reranker=late)`` WITHOUT a text forward pass: the ordinary ``search`` for ``max(fetch,
        top_k)`` hits, then the MaxSim of the query's token matrix with the hits' STORED matrices
        (``IndexFlat.maxsim_ids``), and the ``top_k`` best by that score, best first; ties keep the plain search's
        order.  The result is that of ``search_reranked`` with a ``LateInteraction``, order and score bits, because the
        stored matrices are the ones the forward pass would form again.  A hit without a kept token scores ``-inf``."""
        self._require("late-interaction re-ranking", "set_tokens", "maxsim_ids")
        cfg = config or SearchConfig()
        if cfg.top_k <= 0:
            return []
        n = max(int(fetch), cfg.top_k)
        wide = SearchConfig(top_k=n, similarity_threshold=cfg.similarity_threshold, include_metadata=cfg.include_metadata,
                            include_text=cfg.include_text, max_results=max(cfg.max_results, n))
        with self._lock:
            hits = self.search(query_embedding, wide, filters)
            if not hits:
                return []
            self._sync_tokens(self.faiss_index.ntotal, late)
            q_mat = late.encode_queries([query_text or ""])[0][0]
            ids = np.asarray([self.chunk_id_to_faiss_id[h.chunk_id] for h in hits], dtype=np.int64)
            scores = np.asarray(self.faiss_index.maxsim_ids(q_mat, ids), dtype=np.float32).reshape(-1)
        return [Reranked(hits[int(i)], float(scores[i]), int(i)) for i in np.argsort(-scores, kind="stable")[:cfg.top_k]]

    def search_late_reranked_many(self, query_texts: Sequence[str], query_embeddings, late,
                                  config: Optional[SearchConfig] = None, filters: Optional[Dict[str, Any]] = None,
                                  fetch: int = 50) -> List[List[Reranked]]:
        """``search_late_reranked`` for several queries at once, both stages inside the index: ONE
        ``late.encode_queries`` call (each query in a forward pass of its own, as ``search_late_reranked`` encodes it),
        ONE allow mask and one ``IndexFlat.search_rerank_maxsim`` per 1024 queries -- the dense search for the
        ``max(fetch, top_k)`` best rows of every query, their MaxSim with the stored matrices in one kernel launch and
        the ranking, with ``floor = similarity_threshold``; no id travels through the host between the stages.
        On a store without tombstones and without filters (inner-product similarities, ``top_k <= 128``, every chunk
        with at least one kept token) element ``i`` equals ``search_late_reranked(query_texts[i], query_embeddings[i],
        late, config, fetch=fetch)`` in chunk ids, score bits and ``rank_before``.  Where the two differ:
        tombstoned rows never enter the pool here -- they are always in the allow mask, so the pool holds ``fetch``
        LIVE rows, where ``search_late_reranked`` without ``filter_pushdown`` lets a deleted row take a place of the
        pool and drops it afterwards; ``filters`` are always pushed down into the mask, where ``search_late_reranked``
        without ``filter_pushdown`` filters the best ``max_results`` rows on the host; a hit whose stored matrix is
        empty is left out, where ``search_late_reranked`` returns it last with ``-inf``; the pool is at most 2048
        rows and ``top_k`` at most 128."""
        self._require("late-interaction re-ranking", "set_tokens", "search_rerank_maxsim")
        texts = [t or "" for t in query_texts]
        if not texts:
            return []
        with self._lock:
            frame = self._search_frame(config)
            if frame is None or frame[0].top_k <= 0:
                return [[] for _ in texts]
            cfg, ntotal, _ = frame
            Q = np.ascontiguousarray(np.asarray(query_embeddings, dtype=np.float32).reshape(len(texts), -1))
            n = min(max(int(fetch), cfg.top_k), fi.MAX_K)
            k = max(1, min(cfg.top_k, n, fi.MAX_HYBRID_K))
            tombstones = len(self.faiss_id_to_chunk_id) < ntotal
            allow = self._mask_of(filters or {}, ntotal) if (filters or tombstones) else None
            # the smallest float32 that is no less than the threshold: `s < floor` is then `s < threshold` for every float32 s
            with np.errstate(over="ignore"):
                floor = np.float32(cfg.similarity_threshold)
                if float(floor) < float(cfg.similarity_threshold):
                    floor = np.nextafter(floor, np.float32(np.inf))
            self._sync_tokens(ntotal, late)
            # (one query per forward pass: the encoder picks its tiling by the tokens of a batch, so a query encoded
            # beside others can differ in the last bits of its bf16 tokens from the matrix search_late_reranked forms)
            q_mats = late.encode_queries(texts, batch_size=1)[0]
            out: List[List[Reranked]] = []
            for b0 in range(0, len(texts), fi.MAX_MAXSIM_QUERIES):
                b1 = min(b0 + fi.MAX_MAXSIM_QUERIES, len(texts))
                D, I, S, R = self.faiss_index.search_rerank_maxsim(Q[b0:b1], q_mats[b0:b1], k, n,
                                                                   normalize=self.config.normalize_embeddings,
                                                                   floor=float(floor), allow=allow)
                for b in range(b1 - b0):
                    hits: List[Reranked] = []
                    for d, fid, s, r in zip(D[b].tolist(), I[b].tolist(), S[b].tolist(), R[b].tolist()):
                        chunk_id = self.faiss_id_to_chunk_id.get(fid) if fid >= 0 else None
                        data = self._get_chunk_data(chunk_id) if chunk_id else None
                        if data:
                            hits.append(Reranked(self._make_result(chunk_id, s, data, cfg), float(d), int(r)))
                    out.append(hits)
            return out

    @staticmethod
    def _make_result(chunk_id: str, score: float, data: Dict[str, Any], cfg: SearchConfig) -> SearchResult:
        res = SearchResult(chunk_id=chunk_id, similarity=float(score))
        meta = None
        if cfg.include_metadata:
            meta = json.loads(data["metadata"]) if data["metadata"] else {}
            res.metadata = meta
        if cfg.include_text:
            res.text = data["text"]
        if cfg.include_metadata and cfg.include_text:
            res.chunk = Chunk(id=chunk_id, text=data["text"], metadata=dict(meta), embedding=None)
        return res

    def search_range(self, query_embedding, threshold: Optional[float] = None, filters: Optional[Dict[str, Any]] = None,
                     config: Optional[SearchConfig] = None, limit: Optional[int] = None) -> List[SearchResult]:
        """EVERY live chunk with ``similarity >= threshold`` (default ``config.similarity_threshold``) that matches
        ``filters``, best first -- not capped by ``max_results`` / ``top_k`` as ``search()`` is, only by ``limit`` when
        given.  An L2 storage (``normalize_embeddings=False``) reports squared distances, so there the meaning is
        ``distance <= threshold``, nearest first.  The index call is strict (``IndexFlat.range_search``, faiss'
        comparison): it is handed the neighbouring float32 of the threshold, which makes ``>=`` / ``<=`` exact.
        Tombstones and filters go into the allow mask with ``filter_pushdown``, otherwise the hits are filtered
        afterwards exactly as in ``search()``; both give the same list (no over-fetch is involved here)."""
        cfg = config or SearchConfig()
        thr = float(cfg.similarity_threshold if threshold is None else threshold)
        if thr != thr:
            raise ValueError("search_range: the threshold is NaN")
        if limit is not None and limit <= 0:
            return []
        with self._lock:
            frame = self._search_frame(cfg, query_embedding)
            if frame is None:
                return []
            _, ntotal, q = frame
            radius = strict_radius(thr, bool(self.config.normalize_embeddings))
            allow = self._allow_for(filters, ntotal, tombstones_always=False)
            _, sims, ids = self.faiss_index.range_search(q, float(radius), normalize=self.config.normalize_embeddings,
                                                         allow=allow)
            return self._results_in_rank_order(sims.tolist(), ids.tolist(), cfg, filters, unbounded=True, limit=limit)

    def _facet_buckets(self, by: str, ntotal: int):
        """``(ids, values)`` of a facet over a column or a date unit: ``ids`` int32 ``[ntotal]``, the dense bucket of
        every index row in order of first appearance, ``-1`` for a row whose value is NULL (or whose timestamp does not
        parse) and for a row without a live chunk; ``values[b]`` what bucket ``b`` stands for.  One pass over the
        chunks table, cached per ``by`` under the stamp of ``_allow_mask``."""
        stamp = (self._mutations, len(self.faiss_id_to_chunk_id), ntotal, self.total_chunks)
        hit = self._facet_cache.get(by)
        if hit is not None and hit[0] == stamp:
            return hit[1], hit[2]
        if not self.db:
            raise RuntimeError("Database not initialized")
        ids = np.full(ntotal, -1, dtype=np.int32)
        dense: Dict[Any, int] = {}
        column = "timestamp" if by in FACET_DATES else by
        for cid, value in self.db.cursor().execute(f"SELECT id, {column} FROM chunks"):
            fid = self.chunk_id_to_faiss_id.get(cid)
            if fid is None or fid >= ntotal or self.faiss_id_to_chunk_id.get(fid) != cid:
                continue
            if by in FACET_DATES:
                value = facet_date_key(timestamp_days(value), by)
            elif value is not None and by in ("has_code", "has_tools"):
                value = bool(value)
            if value is not None:
                ids[fid] = dense.setdefault(value, len(dense))
        values = [facet_date_value(v, by) for v in dense] if by in FACET_DATES else list(dense)
        self._facet_cache[by] = (stamp, ids, values)
        return ids, values

    def facets(self, query_embedding, by: str = "project_name", threshold: Optional[float] = None,
               filters: Optional[Dict[str, Any]] = None, config: Optional[SearchConfig] = None,
               top: Optional[int] = None) -> Facets:
        """Where the matches of a query lie: the live chunks with ``similarity >= threshold`` (default
        ``config.similarity_threshold``; an L2 storage: ``distance <= threshold``, as in ``search_range``, made exact
        through the neighbouring float32) that match ``filters``, COUNTED per value of ``by`` inside the index
        (``IndexFlat.facets``: a histogram, no hit list) -- the distribution behind the ``project`` / ``session`` /
        date filters.  ``by`` is a column (``project_name``, ``session_id``, ``chunk_type``, ``has_code``,
        ``has_tools``) or a date unit (``day``, ``week`` starting Monday, ``month``; the chunk's ``timestamp`` in UTC,
        reported as the ISO date of the bucket's first day); anything else raises ``ValueError``.

        Returns ``Facets(total, missing, buckets)``: all matching chunks, those without a value (NULL column, no or
        unparseable timestamp), and one ``Facet(value, count, best)`` per non-empty bucket -- ``best`` the best matching
        chunk of the bucket as ``search()`` would report it under ``config`` -- ordered by count descending, then the
        better best hit, then value, cut to ``top`` when given.

        Tombstones are always masked, and ``filters`` ALWAYS go into the allow mask, whatever ``filter_pushdown`` says:
        a count cannot be filtered afterwards.  ``session_id`` counts over the stored session labels of
        ``search_sessions`` and uploads nothing; every other ``by`` uploads its bucket column (4 bytes per row) with
        the call.  More than ``MAX_FACET_BUCKETS`` distinct values raise ``ValueError``; an index object without
        ``facets`` raises ``NotImplementedError``."""
        if by not in FACET_COLUMNS + FACET_DATES:
            raise ValueError(f"facets: by={by!r} is not one of {', '.join(FACET_COLUMNS + FACET_DATES)}")
        cfg = config or SearchConfig()
        thr = float(cfg.similarity_threshold if threshold is None else threshold)
        if thr != thr:
            raise ValueError("facets: the threshold is NaN")
        self._require("facet counts", "facets", *(("set_groups",) if by == "session_id" else ()))
        with self._lock:
            frame = self._search_frame(cfg, query_embedding)
            if frame is None:
                return Facets(0, 0, [])
            _, ntotal, q = frame
            similarity = bool(self.config.normalize_embeddings)
            radius = strict_radius(thr, similarity)
            by_attribute = None
            if by in DICT_COLUMNS + FLAG_COLUMNS and self._attribute_path():
                self._sync_attributes(ntotal)
                # the codes ARE dense bucket ids, NULL = -1 = unbucketed.  The dictionary keeps the values of deleted
                # chunks until the next compaction: where it is larger than the index takes, the upload path below
                # decides over the live values alone, as with the option off
                if not self._catalog.mixed[by] and len(self._catalog.values(by)) <= fi.MAX_FACET_BUCKETS:
                    by_attribute = self._catalog.slot(by)
            if by_attribute is not None:
                ids, values = None, self._catalog.values(by)
            elif by == "session_id":
                self._sync_session_labels(ntotal)
                ids, values = None, list(self._session_labels)   # (label = position: dense in order of first appearance)
            else:
                ids, values = self._facet_buckets(by, ntotal)
            if len(values) > fi.MAX_FACET_BUCKETS:
                raise ValueError(f"facets: by={by!r} has {len(values)} distinct values, more than {fi.MAX_FACET_BUCKETS}")
            allow = self._mask_of(filters or {}, ntotal)
            more = {} if by_attribute is None else {"by_attribute": by_attribute}
            res = self.faiss_index.facets(q, float(radius), buckets=ids, nbuckets=max(len(values), 1),
                                          normalize=self.config.normalize_embeddings,
                                          allow=None if bool(allow.all()) else allow, **more)
            out = []
            for b in np.flatnonzero(res.counts[0] > 0).tolist():
                chunk_id = self.faiss_id_to_chunk_id.get(int(res.best_id[0, b]))
                data = self._get_chunk_data(chunk_id) if chunk_id else None
                if data:
                    out.append(Facet(values[b], int(res.counts[0, b]),
                                     self._make_result(chunk_id, float(res.best_score[0, b]), data, cfg)))
            return Facets(int(res.total[0]), int(res.unbucketed[0]), order_facets(out, similarity, top))

    def _allow_mask(self, filters: Dict[str, Any], ntotal: int) -> np.ndarray:
        """Boolean mask over index rows: live (not tombstoned) and matching ``filters`` under exactly the
        semantics of ``_matches_filters``.  One pass over the chunks table, cached until the id maps change."""
        key = json.dumps(filters, sort_keys=True, default=str)
        hit = self._allow_cache.get(key)
        stamp = (self._mutations, len(self.faiss_id_to_chunk_id), ntotal, self.total_chunks)
        if hit is not None and hit[0] == stamp:
            return hit[1]
        allow = np.zeros(ntotal, dtype=bool)
        if not self.db:
            raise RuntimeError("Database not initialized")
        for row in self.db.cursor().execute("SELECT * FROM chunks"):
            fid = self.chunk_id_to_faiss_id.get(row["id"])
            if fid is None or fid >= ntotal or self.faiss_id_to_chunk_id.get(fid) != row["id"]:
                continue
            if filters and not self._matches_filters({k_: row[k_] for k_ in row.keys()}, filters):
                continue
            allow[fid] = True
        if len(self._allow_cache) >= 8:
            self._allow_cache.clear()
        self._allow_cache[key] = (stamp, allow)
        return allow

    def _get_chunk_data(self, chunk_id: str) -> Optional[Dict[str, Any]]:
        if not self.db:
            raise RuntimeError("Database not initialized")
        row = self.db.cursor().execute("SELECT * FROM chunks WHERE id = ?", (chunk_id,)).fetchone()
        return {key: row[key] for key in row.keys()} if row else None

    _RANGE_OPS = {
        "gte": lambda v, b: v >= b,
        "lte": lambda v, b: v <= b,
        "gt": lambda v, b: v > b,
        "lt": lambda v, b: v < b,
    }

    def _matches_filters(self, chunk_data: Dict[str, Any], filters: Dict[str, Any]) -> bool:
        """Range dict / list-IN / case-insensitive substring for project_name /
        exact otherwise; keys absent from the row are ignored (``src/storage.py:508-543``)."""
        for key, want in filters.items():
            if key not in chunk_data:
                continue
            have = chunk_data[key]
            if isinstance(want, dict):
                for op, bound in want.items():
                    test = self._RANGE_OPS.get(op)
                    if test is not None and not test(have, bound):
                        return False
            elif isinstance(want, list):
                if have not in want:
                    return False
            elif key == "project_name" and isinstance(want, str) and isinstance(have, str):
                if want.lower() not in have.lower():
                    return False
            elif have != want:
                return False
        return True

    # ------------------------------------------------------------- metadata
    def get_chunk_by_id(self, chunk_id: str) -> Optional[Chunk]:
        if not self.db:
            raise RuntimeError("Database not initialized")
        data = self._get_chunk_data(chunk_id)
        if not data:
            return None
        meta = json.loads(data["metadata"]) if data["metadata"] else {}
        return Chunk(id=chunk_id, text=data["text"], metadata=meta, embedding=None)

    def _chunks_where(self, column: str, value: str) -> List[Chunk]:
        if not self.db:
            raise RuntimeError("Database not initialized")
        cur = self.db.cursor()
        cur.execute(f"SELECT * FROM chunks WHERE {column} = ? ORDER BY timestamp", (value,))
        return [_row_to_chunk(r) for r in cur.fetchall()]

    def get_chunks_by_session(self, session_id: str) -> List[Chunk]:
        return self._chunks_where("session_id", session_id)

    def get_chunks_by_project(self, project_name: str) -> List[Chunk]:
        return self._chunks_where("project_name", project_name)

    def delete_chunk(self, chunk_id: str) -> bool:
        self._mutations += 1  # invalidates cached allow masks (filter push-down)
        with self._lock:
            fid = self.chunk_id_to_faiss_id.get(chunk_id)
            if fid is None:
                return False
            cur = self.db.cursor()
            cur.execute("DELETE FROM chunks WHERE id = ?", (chunk_id,))
            if cur.rowcount == 0:
                return False
            # the vector stays in the index as a tombstone (reference behaviour)
            del self.chunk_id_to_faiss_id[chunk_id]
            del self.faiss_id_to_chunk_id[fid]
            self.db.commit()
            self.total_chunks -= 1
            return True

    def delete_chunks_by_session(self, session_id: str) -> int:
        self._mutations += 1  # invalidates cached allow masks (filter push-down)
        if not self.db:
            raise RuntimeError("Database not initialized")
        cur = self.db.cursor()
        cur.execute("SELECT id FROM chunks WHERE session_id = ?", (session_id,))
        return sum(1 for (cid,) in cur.fetchall() if self.delete_chunk(cid))

    def get_stats(self) -> Dict[str, Any]:
        if not self.db:
            raise RuntimeError("Database not initialized")
        cur = self.db.cursor()
        one = lambda sql: cur.execute(sql).fetchone()[0]  # noqa: E731
        total_chunks = one("SELECT COUNT(*) FROM chunks")
        total_sessions = one("SELECT COUNT(DISTINCT session_id) FROM chunks")
        total_projects = one("SELECT COUNT(DISTINCT project_name) FROM chunks")
        chunk_types = dict(cur.execute("SELECT chunk_type, COUNT(*) FROM chunks GROUP BY chunk_type").fetchall())
        try:
            projects = self.get_all_projects()
        except Exception as e:
            self.logger.warning(f"Failed to get projects list: {e}")
            projects = []
        index_bytes = self.index_path.stat().st_size if self.index_path.exists() else 0
        db_bytes = self.db_path.stat().st_size if self.db_path.exists() else 0
        stats: Dict[str, Any] = {
            "total_chunks": total_chunks,
            "total_sessions": total_sessions,
            "total_projects": total_projects,
            "projects": projects,
            "chunk_types": chunk_types,
            "faiss_index_size": index_bytes,
            "database_size": db_bytes,
            "total_storage_size": index_bytes + db_bytes,
            "embedding_dimension": self.embedding_dim,
            "index_type": self.config.index_type,
            "use_gpu": self.config.use_gpu,
            "is_gpu_index": self._is_gpu_index,
        }
        cap = self._gpu_capability
        if cap:
            info = {
                "gpu_available": cap.can_use_gpu,
                "gpu_count": cap.gpu_count,
                "gpu_names": cap.gpu_names,
                "status_message": cap.status_message,
            }
            if cap.gpu_memory_total is not None:
                info["gpu_memory_total_gb"] = cap.gpu_memory_total / (1024**3)
            if cap.gpu_memory_free is not None:
                info["gpu_memory_free_gb"] = cap.gpu_memory_free / (1024**3)
            stats["gpu_info"] = info
        return stats

    def get_all_projects(self) -> List[str]:
        if not self.db:
            raise RuntimeError("Database not initialized. Call initialize() first.")
        cur = self.db.cursor()
        cur.execute(
            "SELECT DISTINCT project_name FROM chunks "
            "WHERE project_name IS NOT NULL AND project_name != '' ORDER BY project_name"
        )
        return [r[0] for r in cur.fetchall()]

    # --------------------------------------------------------- file tracking
    def update_file_info(self, file_path: str, chunk_count: int) -> None:
        if not self.db:
            raise RuntimeError("Database not initialized")
        try:
            modified = datetime.fromtimestamp(os.path.getmtime(file_path))
        except OSError:
            modified = datetime.now()
        self.db.cursor().execute(
            "INSERT OR REPLACE INTO files (path, last_modified, last_indexed, chunk_count) VALUES (?, ?, ?, ?)",
            (file_path, modified, datetime.now(), chunk_count),
        )
        self.db.commit()

    def is_file_modified(self, file_path: str) -> bool:
        try:
            current = datetime.fromtimestamp(os.path.getmtime(file_path))
        except OSError:
            return True
        row = self.db.cursor().execute(
            "SELECT last_modified, last_indexed FROM files WHERE path = ?", (file_path,)
        ).fetchone()
        if not row or not row["last_modified"]:
            return True
        return current > datetime.fromisoformat(row["last_modified"])

    def remove_chunks_for_file(self, file_path: str) -> int:
        self._mutations += 1  # invalidates cached allow masks (filter push-down)
        with self._lock:
            cur = self.db.cursor()
            doomed = cur.execute("SELECT id, faiss_id FROM chunks WHERE file_path = ?", (file_path,)).fetchall()
            if not doomed:
                return 0
            cur.execute("DELETE FROM chunks WHERE file_path = ?", (file_path,))
            self.db.commit()
            for row in doomed:
                self.chunk_id_to_faiss_id.pop(row["id"], None)
                if row["faiss_id"] is not None:
                    self.faiss_id_to_chunk_id.pop(row["faiss_id"], None)
            return len(doomed)

    def clear_all_data(self) -> None:
        self._mutations += 1  # invalidates cached allow masks (filter push-down)
        with self._lock:
            self.faiss_index = self._create_cpu_index()
            self._saved_rows = -1
            cur = self.db.cursor()
            cur.execute("DELETE FROM chunks")
            cur.execute("DELETE FROM files")
            self.db.commit()
            self.chunk_id_to_faiss_id.clear()
            self.faiss_id_to_chunk_id.clear()
            self.total_chunks = 0
            self._drop_sparse_file()
            self._drop_tokens_file()
            if self.config.auto_save:
                self.save_index()
        self.logger.info("Cleared all data from storage")

    # ---------------------------------------------------------- persistence
    def save_index(self) -> None:
        """Write ``embeddings.faiss`` (IndexFlat on-disk layout).  When the file
        already holds the first ``_saved_rows`` rows only the new rows are appended
        and the two counters in the header are patched."""
        if not self.faiss_index:
            self.logger.warning("No FAISS index to save")
            return
        with self._lock:
            ix = self.faiss_index
            n = ix.ntotal
            path = str(self.index_path)
            if 0 <= self._saved_rows <= n and self.index_path.exists() and self._saved_rows > 0:
                if n > self._saved_rows:
                    new_rows = ix.reconstruct_n(self._saved_rows, n - self._saved_rows)
                    with open(path, "r+b") as f:
                        # rows first, made durable, THEN the two header counters: a crash in between leaves a
                        # file whose header still describes the old, complete prefix (trailing bytes are ignored
                        # by read_index), never a header that promises rows the file does not hold
                        f.seek(_INDEX_HEADER_BYTES + self._saved_rows * ix.d * 4)
                        f.write(new_rows.tobytes())
                        f.truncate()
                        f.flush()
                        os.fsync(f.fileno())
                        f.seek(8)
                        f.write(struct.pack("<q", n))
                        f.seek(8 + 8 + 16 + 1 + 4)
                        f.write(struct.pack("<Q", n * ix.d))
                        f.flush()
                        os.fsync(f.fileno())
            else:
                self._write_index_atomically(ix, path)
            self._saved_rows = n
            self._save_sparse(n)
            self._save_tokens(n)
        self.logger.info(f"Saved flat index ({n} vectors) to {self.index_path}")

    def _crash_point(self, where: str) -> None:
        """Test seam: tests replace this to simulate a crash between the steps of a journaled operation."""

    @staticmethod
    def _write_index_atomically(ix, path: str) -> None:
        """Whole-file write through a temporary sibling + ``os.replace``: readers (and a crash) see the old file or
        the new one, never a torn one; the directory entry is made durable too."""
        tmp = path + ".tmp"
        fi.write_index(ix, tmp)
        with open(tmp, "rb") as f:
            os.fsync(f.fileno())
        os.replace(tmp, path)
        _fsync_dir(Path(path).parent)

    def backup(self, backup_dir: str) -> None:
        dest = Path(backup_dir)
        dest.mkdir(parents=True, exist_ok=True)
        if self.faiss_index and self.faiss_index.ntotal > 0:
            fi.write_index(self.faiss_index, str(dest / self.config.index_name))
        if self.db_path.exists() and self.db:
            target = sqlite3.connect(str(dest / self.config.db_name))
            self.db.backup(target)
            target.close()
        self.logger.info(f"Backup created in {dest}")

    def restore(self, backup_dir: str) -> None:
        self._mutations += 1  # invalidates cached allow masks (filter push-down)
        src = Path(backup_dir)
        with self._lock:
            ipath = src / self.config.index_name
            if ipath.exists():
                self.faiss_index = self._read_index(str(ipath))
                self._saved_rows = -1
            dpath = src / self.config.db_name
            if dpath.exists():
                self.db.close()
                self.db = sqlite3.connect(str(self.db_path), check_same_thread=False)
                self.db.row_factory = sqlite3.Row
                source = sqlite3.connect(str(dpath))
                source.backup(self.db)
                source.close()
            self._rebuild_id_mappings()
        self.logger.info(f"Restored from backup in {src}")

    def optimize(self) -> None:
        self.logger.info("Optimizing storage...")
        self.db.execute("VACUUM")
        if self.total_chunks != self.faiss_index.ntotal:
            self.logger.info("Rebuilding flat index...")
            self._rebuild_faiss_index()
        self.logger.info("Storage optimization complete")

    def _rebuild_faiss_index(self) -> None:
        """Compact tombstones: keep only rows still referenced by SQLite, in
        faiss_id order, and renumber.  (The reference leaves this as a stub that
        would drop every vector, ``src/storage.py:944-969``; the vectors are
        available here because the index can export its rows.)"""
        with self._lock:
            cur = self.db.cursor()
            live = cur.execute(
                "SELECT id, faiss_id FROM chunks WHERE faiss_id IS NOT NULL ORDER BY faiss_id"
            ).fetchall()
            if not live:
                return
            old = self.faiss_index
            ids = [r["faiss_id"] for r in live]
            # An index that can drop rows in place (IndexFlat.remove_ids) is compacted where it lies: the compacted
            # file is streamed from its live rows and the index itself shrinks only once both files have changed.
            # Others (the sharded facade) are rebuilt into a second index.
            in_place = hasattr(old, "remove_ids")
            fresh = None
            if not in_place:
                fresh = self._create_cpu_index()
                fresh.reserve(len(live))
                step = 1 << 16
                for s in range(0, len(ids), step):
                    part = ids[s:s + step]
                    lo, hi = part[0], part[-1] + 1
                    block = old.reconstruct_n(lo, hi - lo)
                    fresh.add(block[np.asarray(part) - lo])  # already normalised
            fwd: Dict[str, int] = {}
            rev: Dict[int, str] = {}
            updates = []
            for new_id, row in enumerate(live):
                fwd[row["id"]] = new_id
                rev[new_id] = row["id"]
                updates.append((new_id, row["id"]))
            # The renumbered ids only make sense with the compacted rows, whatever auto_save says.  Two files cannot
            # change atomically together, so the step is journaled (see _recover_interrupted_compaction): compacted
            # file beside the index, then ONE transaction with the new ids + a flag, then the rename, then the flag
            # is cleared.  A crash at any point leaves a state the next initialize() completes or discards.
            compact = str(self.index_path) + ".compact"
            if in_place:
                self._write_index_atomically(_LiveRows(old, ids), compact)
            else:
                self._write_index_atomically(fresh, compact)
            cur.executemany("UPDATE chunks SET faiss_id = ? WHERE id = ?", updates)
            cur.execute("INSERT OR REPLACE INTO storage_meta (key, value) VALUES ('pending_compact', ?)", (str(len(live)),))
            self.db.commit()
            self._crash_point("compaction committed, file not yet moved")
            self._drop_sparse_file()            # (it speaks the old numbering)
            self._drop_tokens_file()
            os.replace(compact, str(self.index_path))
            _fsync_dir(self.index_path.parent)
            cur.execute("DELETE FROM storage_meta WHERE key = 'pending_compact'")
            self.db.commit()
            if in_place:                        # (the live index shrinks only once both files have changed)
                dead = np.ones(old.ntotal, dtype=np.bool_)
                dead[np.asarray(ids, dtype=np.int64)] = False
                old.remove_ids(np.flatnonzero(dead))
            self.chunk_id_to_faiss_id = fwd     # (in-memory maps change only once both files have)
            self.faiss_id_to_chunk_id = rev
            if not in_place:
                self.faiss_index = fresh
            self._saved_rows = self.faiss_index.ntotal
            self.total_chunks = len(live)
            self._mutations += 1
            # (the rows were renumbered: search_sessions, search_recent and search_hybrid push every row again)
            self._labels, self._priors, self._terms = _Synced(), _Synced(), _Synced()
            self._attrs = _Synced()
            # ... but no text is encoded again: an index compacted in place has compacted its sparse vectors with the rows
            if in_place and self._sparse.index is old and hasattr(old, "sparse_rows"):
                self._sparse.rows = int(old.sparse_rows)
            else:
                self._sparse = _Synced()
            if in_place and self._tokens.index is old and hasattr(old, "token_rows"):   # (and its token matrices)
                self._tokens.rows = int(old.token_rows)
            else:
                self._tokens = _Synced()
            if self.config.auto_save:
                self._save_sparse(self.faiss_index.ntotal)
                self._save_tokens(self.faiss_index.ntotal)
            if not in_place:
                old.close()
        self.logger.info("Flat index rebuilt")

    def close(self) -> None:
        if self.config.auto_save:
            self.save_index()
        if self.db:
            self.db.close()
        self.logger.info("Storage closed")

    def __enter__(self) -> "HybridStorage":
        self.initialize()
        return self

    def __exit__(self, exc_type: Any, exc_val: Any, exc_tb: Any) -> None:
        self.close()
