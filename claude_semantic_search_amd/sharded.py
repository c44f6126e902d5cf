"""Row-partitioned flat index across the GPUs of one node.

One process per GPU (``torch.distributed``; backend "nccl" is RCCL on ROCm).  Every rank keeps its rows in its
own HBM as an ordinary ``IndexFlat``.  A search is: every rank sweeps its shard for the (replicated) query batch
-> ONE all-gather of the per-shard top-k, ids and scores packed into a single buffer of ``nq*k*12`` bytes per
rank (latency bound, nothing bulky ever crosses xGMI) -> every rank merges the ``G*k`` candidates per query by
(score, id).  There is no reference counterpart (the reference pins faiss to device 0, ``src/storage.py:283``);
semantics are those of one big ``IndexFlat`` and are tested as such.

Rows enter through collective calls (every rank passes the same arguments, no communication needed):

* ``add_global(x)`` / ``add_synthetic_global(n)``: the call's rows are split into ``world`` contiguous blocks,
  rank ``r`` keeps block ``r``;
* ``add_routed(x)``: an incremental add (a file's worth of chunks) goes whole to the least-full shard.

Global ids are insertion order over the calls, exactly as one ``IndexFlat`` would number them
(``src/storage.py:358-365``).  A shard therefore holds a list of segments ``(local_row0, global_row0, n)``; with one
segment the library's ``id_base`` does the translation inside the search kernels, with several the local ids are
mapped through the segment table after the local search.

The communication skeleton is backend agnostic (the CPU tests run it over gloo with test doubles for the device
pieces); the product wiring uses device buffers end to end.
"""
from __future__ import annotations

import ctypes
from typing import Callable, List, Optional, Tuple

import numpy as np


def shard_bounds(n_total: int, world: int, rank: int) -> Tuple[int, int]:
    """Contiguous, balanced row partition: rows [lo, hi) of rank `rank`."""
    return rank * n_total // world, (rank + 1) * n_total // world


def packed_layout(nq: int, k: int) -> Tuple[int, int, int]:
    """Per-rank exchange record: ``[nq*k int64 ids][nq*k float32 scores]`` padded to 16 bytes.
    Returns (bytes of the id part, bytes of ids + scores, padded record size)."""
    n = nq * k
    return 8 * n, 12 * n, (12 * n + 15) // 16 * 16


class ShardedFlatIndex:
    """``IndexFlat`` semantics over ``world`` row shards.

    ``local_index`` must offer ``ntotal``, ``add(x, normalize=)``, ``add_synthetic``, ``set_id_base`` and
    ``search_dev``/``search`` (``range_search`` for ``range_search``, ``reconstruct_n`` for ``search_by_ids`` and ``search_diverse``; ``kmeans_step``, ``bounds`` and ``reconstruct_batch`` for ``kmeans``; ``subset_terms`` and ``term_stats`` for ``significant_terms``; ``facets`` for ``facets``); ``merge`` merges ``[world, nq, k]`` candidate tensors.  Defaults are the HIP
    implementations; tests substitute doubles.
    """

    def __init__(self, d: int, metric: int = 0, group=None, device_index: Optional[int] = None,
                 index_factory: Optional[Callable] = None, merge: Optional[Callable] = None):
        import torch.distributed as dist

        self.dist = dist
        self.group = group
        self.rank = dist.get_rank(group) if dist.is_initialized() else 0
        self.world = dist.get_world_size(group) if dist.is_initialized() else 1
        self.d, self.metric = int(d), int(metric)
        self.device_index = device_index
        if index_factory is None:
            from .flat_index import IndexFlat

            index_factory = lambda: IndexFlat(self.d, self.metric, device=device_index or 0)  # noqa: E731
        self.local = index_factory()
        self._merge = merge      # None: the HIP merge straight from the packed exchange buffer
        #: run the all-gather + merge even with ONE rank (tests: the RCCL calls of the N > 1 path on a one-GPU box)
        self.exchange_when_single = False
        self.ntotal_global = 0
        self.shard_sizes = [0] * self.world          # replicated bookkeeping (all adds are collective calls)
        self.segments: List[Tuple[int, int, int]] = []   # (local_row0, global_row0, n) of THIS shard
        self._seg_tensors = None
        self._dead: Optional[np.ndarray] = None          # tombstones in global numbering (replicated; mark_deleted)
        self._terms_global = 0                           # leading GLOBAL rows that have term lists (replicated; set_terms)
        self._sparse_global = 0                          # ... that have sparse vectors (replicated; set_sparse)
        self._tokens_global = 0                          # ... that have token matrices, and their width (set_tokens)
        self._token_dim = 0
        self._attr_types: dict = {}                      # slot -> type of the attribute columns (replicated; set_attribute)

    # -- building ----------------------------------------------------------
    def _append_segment(self, n_local: int, global_row0: int) -> None:
        if n_local <= 0:
            return
        local_row0 = self.shard_sizes[self.rank]
        if self.segments and self.segments[-1][0] + self.segments[-1][2] == local_row0 and \
                self.segments[-1][1] + self.segments[-1][2] == global_row0:
            l0, g0, n0 = self.segments[-1]
            self.segments[-1] = (l0, g0, n0 + n_local)       # contiguous in both numberings: one segment
        else:
            self.segments.append((local_row0, global_row0, n_local))
        # one segment: the kernels add id_base themselves; several: local ids, translated after the search
        self.local.set_id_base(self.segments[0][1] - self.segments[0][0] if len(self.segments) == 1 else 0)
        self._seg_tensors = None

    def _account(self, counts: List[int], n_call: int) -> None:
        for r, c in enumerate(counts):
            self.shard_sizes[r] += c
        self.ntotal_global += n_call

    def add_global(self, x: np.ndarray, normalize: bool = False) -> None:
        """Every rank passes the same full ``x``; rank r keeps the r-th contiguous block of the call's rows."""
        n = int(x.shape[0])
        bounds = [shard_bounds(n, self.world, r) for r in range(self.world)]
        lo, hi = bounds[self.rank]
        if hi > lo:
            self.local.add(np.ascontiguousarray(x[lo:hi]), normalize=normalize)
        self._append_segment(hi - lo, self.ntotal_global + lo)
        self._account([b[1] - b[0] for b in bounds], n)

    def add_routed(self, x: np.ndarray, normalize: bool = False) -> int:
        """Incremental add: the whole call goes to the least-full shard (lowest rank on ties).  Returns that rank."""
        n = int(x.shape[0])
        target = min(range(self.world), key=lambda r: (self.shard_sizes[r], r))
        if n and target == self.rank:
            self.local.add(np.ascontiguousarray(x), normalize=normalize)
            self._append_segment(n, self.ntotal_global)
        counts = [0] * self.world
        counts[target] = n
        self._account(counts, n)
        return target

    def add_synthetic_global(self, n_total: int, seed: int, normalize: bool = True, stream: int = 0) -> None:
        """Rows of the virtual synthetic index (``css_synth.h``, row r is the same vector wherever it lives)."""
        bounds = [shard_bounds(n_total, self.world, r) for r in range(self.world)]
        lo, hi = bounds[self.rank]
        if self.shard_sizes[self.rank] == 0:
            self.local.reserve(hi - lo)
        if hi > lo:
            self.local.add_synthetic(hi - lo, seed, first_row=lo, normalize=normalize, stream=stream)
        self._append_segment(hi - lo, self.ntotal_global + lo)
        self._account([b[1] - b[0] for b in bounds], n_total)

    # -- id translation ------------------------------------------------------
    def _to_global(self, I):
        """Local row numbers -> global ids through the segment table (only needed with several segments)."""
        import torch

        if len(self.segments) <= 1:
            return I
        if self._seg_tensors is None or self._seg_tensors[0].device != I.device:
            l0 = torch.tensor([s[0] for s in self.segments], dtype=torch.int64, device=I.device)
            g0 = torch.tensor([s[1] for s in self.segments], dtype=torch.int64, device=I.device)
            self._seg_tensors = (l0, g0)
        l0, g0 = self._seg_tensors
        seg = (torch.bucketize(I, l0, right=True) - 1).clamp_(min=0)
        return torch.where(I >= 0, I - l0[seg] + g0[seg], I)

    def _to_global_np(self, I: np.ndarray) -> np.ndarray:
        """``_to_global`` for a host array of local row numbers; ``-1`` pads stay ``-1``."""
        if len(self.segments) <= 1 or I.size == 0:
            return I
        l0 = np.array([s[0] for s in self.segments], dtype=np.int64)
        g0 = np.array([s[1] for s in self.segments], dtype=np.int64)
        seg = np.clip(np.searchsorted(l0, I, side="right") - 1, 0, None)
        return np.where(I >= 0, I - l0[seg] + g0[seg], I)

    def _overlaps(self, row0: int, n: int):
        """The walk over the segment table: for every segment of THIS shard that overlaps the GLOBAL rows
        ``[row0, row0 + n)``, ``(local row, global row, length)`` of the overlap."""
        for l0, g0, m in self.segments:
            lo, hi = max(g0, row0), min(g0 + m, row0 + n)
            if hi > lo:
                yield l0 + (lo - g0), lo, hi - lo

    def _check_rows(self, what: str, row0: int, n: int) -> None:
        if row0 < 0 or row0 + n > self.ntotal_global:
            raise ValueError(f"{what}: rows [{row0}, {row0 + n}) outside [0, {self.ntotal_global})")

    def _check_ids(self, what: str, ids: np.ndarray) -> None:
        bad = ids[(ids < 0) | (ids >= self.ntotal_global)]
        if bad.size:
            raise ValueError(f"{what}: id {int(bad[0])} outside [0, {self.ntotal_global})")

    # -- pieces of the host-side searches ------------------------------------
    def _queries(self, q) -> np.ndarray:
        return np.ascontiguousarray(q, dtype=np.float32).reshape(-1, self.d)

    def _single(self) -> bool:
        """One rank and no forced exchange: the local answer is the answer."""
        return self.world == 1 and not self.exchange_when_single

    def _exchange_device(self) -> str:
        """Where a host array goes for a collective: gloo moves host memory, RCCL this rank's device."""
        return "cpu" if self.dist.get_backend(self.group) == "gloo" else f"cuda:{self.device_index or 0}"

    def _all_gather_host(self, send: np.ndarray) -> np.ndarray:
        """ONE all-gather of a flat host record (the same size on every rank): ``[world, record]``."""
        import torch

        t = torch.from_numpy(send).to(self._exchange_device())
        recv = torch.empty(self.world * t.shape[0], dtype=t.dtype, device=t.device)
        self.dist.all_gather_into_tensor(recv, t, group=self.group)
        return recv.cpu().numpy().reshape(self.world, t.shape[0])

    def _sum_over_ranks(self, a: np.ndarray) -> np.ndarray:
        """ONE sum all-reduce of a host array (none with one rank, or for nothing)."""
        import torch

        if self.world == 1 or a.size == 0:
            return a
        t = torch.from_numpy(a).to(self._exchange_device())
        self.dist.all_reduce(t, group=self.group)
        return t.cpu().numpy()

    def _owned_rows(self, global_ids: np.ndarray) -> np.ndarray:
        """The stored rows of ``global_ids`` (any shape; ``-1`` = none) on every rank, ``[..., d]``: the shard that
        owns an id supplies its row through the segment table, every other shard zeros, then ``_sum_over_ranks``
        (exact: one non-zero contribution per row)."""
        rows = np.zeros(global_ids.shape + (self.d,), dtype=np.float32)
        for l0, g0, m in self.segments:
            for at in map(tuple, np.argwhere((global_ids >= g0) & (global_ids < g0 + m))):
                rows[at] = self.local.reconstruct_n(l0 + int(global_ids[at]) - g0, 1)[0]
        return self._sum_over_ranks(rows)

    def _best_first(self, scores: np.ndarray, ids: np.ndarray, lead: np.ndarray, metric: Optional[int] = None) -> np.ndarray:
        """Sort order by ``lead`` ascending, then best score first (IP descending, L2 ascending; ``metric``: that of the
        scores where it is not the index's), then ascending id."""
        return np.lexsort((ids, -scores if (self.metric if metric is None else metric) == 0 else scores, lead))

    def _columns(self, I, cols, last=np.float32, metric: Optional[int] = None):
        """The exchange of a local result of fixed-width columns: ``I`` the local ids and ``cols`` the 4-byte columns
        that ride along (float32; the last one ``last``), ``[nq, k]`` or ``[k]`` each.  Returns ``(I, cols, local)``:
        contiguous, ids GLOBAL.  One rank, or no query: the local answer is the answer (``local``, shapes as given).
        Otherwise ONE all-gather of this rank's ``[ids | column ...]`` record, ``8 + 4 * len(cols)`` bytes per entry, and
        every rank's entries side by side per query, ``[nq, world * k]``, best first by ``(cols[0], id)`` with the
        pads last."""
        I = np.ascontiguousarray(self._to_global_np(np.asarray(I, dtype=np.int64)))
        cols = [np.ascontiguousarray(c, dtype=np.float32 if j + 1 < len(cols) else last) for j, c in enumerate(cols)]
        if self._single() or I.size == 0:
            return I, cols, True
        k, n = I.shape[-1], I.size
        send = np.empty((8 + 4 * len(cols)) * n, dtype=np.uint8)
        send[:8 * n] = I.reshape(-1).view(np.uint8)
        for c, a in enumerate(cols):
            send[(8 + 4 * c) * n:(12 + 4 * c) * n] = a.reshape(-1).view(np.uint8)
        recv = self._all_gather_host(send)
        side_by_side = lambda lo, hi, dt: np.concatenate(
            [recv[r, lo * n:hi * n].view(dt).reshape(-1, k) for r in range(self.world)], axis=1)
        Ig = side_by_side(0, 8, np.int64)
        out = [side_by_side(8 + 4 * c, 12 + 4 * c, a.dtype) for c, a in enumerate(cols)]
        for j in range(Ig.shape[0]):
            order = self._best_first(out[0][j], Ig[j], Ig[j] < 0, metric)
            for a in [Ig] + out:
                a[j] = a[j][order]
        return Ig, out, False

    # -- searching ---------------------------------------------------------
    def _merge_packed_hip(self, recv, nq: int, k: int, record: int):
        import torch

        from . import _native as nat

        Dm = torch.empty((nq, k), dtype=torch.float32, device=recv.device)
        Im = torch.empty((nq, k), dtype=torch.int64, device=recv.device)
        st = torch.cuda.current_stream().cuda_stream
        nat.check(nat.lib().css_merge_topk_packed_dev(ctypes.c_void_p(recv.data_ptr()), self.world, record, nq, k,
                                                      self.metric, ctypes.c_void_p(Dm.data_ptr()),
                                                      ctypes.c_void_p(Im.data_ptr()), recv.device.index or 0,
                                                      ctypes.c_void_p(st)))
        return Dm, Im

    # -- allow-masks and tombstones (filter push-down, src/storage.py:438-492, :611-635) --------------------
    def local_rows_of(self, global_mask: np.ndarray) -> np.ndarray:
        """This shard's part of a per-row array in GLOBAL numbering (``ntotal_global`` entries, the same on every
        rank), in local row order -- through the segment table."""
        g = np.asarray(global_mask)
        if g.shape[0] != self.ntotal_global:
            raise ValueError(f"mask has {g.shape[0]} entries, the sharded index {self.ntotal_global} rows")
        out = np.zeros(self.shard_sizes[self.rank], dtype=g.dtype)
        for l0, g0, n in self._overlaps(0, self.ntotal_global):
            out[l0:l0 + n] = g[g0:g0 + n]
        return out

    def mark_deleted(self, global_ids) -> None:
        """Tombstones: rows that no search may return any more (collective: every rank passes the same ids).  The rows
        stay in HBM, as in the reference, until the caller compacts (``HybridStorage._rebuild_faiss_index``)."""
        ids = np.asarray(list(global_ids), dtype=np.int64)
        if ids.size == 0:
            return
        if self._dead is None or self._dead.shape[0] < self.ntotal_global:
            grown = np.zeros(self.ntotal_global, dtype=bool)
            if self._dead is not None:
                grown[: self._dead.shape[0]] = self._dead
            self._dead = grown
        self._dead[ids] = True

    def _local_allow(self, allow) -> Optional[np.ndarray]:
        """Boolean mask over THIS shard's rows: the caller's global allow-mask minus the tombstones (None = every row)."""
        dead = None
        if self._dead is not None and self._dead.any():
            dead = np.zeros(self.ntotal_global, dtype=bool)
            dead[: self._dead.shape[0]] = self._dead
        if allow is None and dead is None:
            return None
        g = np.ones(self.ntotal_global, dtype=bool) if allow is None else np.asarray(allow, dtype=bool)
        if dead is not None:
            g = g & ~dead
        return self.local_rows_of(g)

    def search_tensors(self, q, k: int, normalize: bool = False, allow=None):
        """``q``: [nq, d] float32 tensor on this rank's device (same on all ranks).  ``allow``: optional boolean array
        over the GLOBAL rows (same on all ranks): only rows marked True can be returned; every rank cuts its shard's
        part out and hands it to the local masked search (``css_index_search_masked_dev``).
        Returns merged ``(D, I)`` tensors (global ids) on every rank."""
        import torch

        nq = q.shape[0]
        ib, db, record = packed_layout(nq, k)
        # the local result is written straight into this rank's exchange record: [ids | scores]
        send = torch.empty(record, dtype=torch.uint8, device=q.device)
        I = send[:ib].view(torch.int64).view(nq, k)
        D = send[ib:db].view(torch.float32).view(nq, k)
        loc = self._local_allow(allow)
        if q.is_cuda:
            st = torch.cuda.current_stream().cuda_stream
            bits = None
            if loc is not None and loc.shape[0]:
                from .flat_index import pack_allow_bits

                bits = torch.from_numpy(pack_allow_bits(loc, loc.shape[0]).view(np.int32)).to(q.device)
            self.local.search_dev(q.data_ptr(), nq, k, D.data_ptr(), I.data_ptr(), st, normalize=normalize,
                                  allow_bits_ptr=bits.data_ptr() if bits is not None else 0)
            if bits is not None:
                bits.record_stream(torch.cuda.current_stream())
        else:  # CPU doubles (tests)
            d_np, i_np = self.local.search(q.numpy(), k, normalize=normalize, allow=loc)
            D.copy_(torch.from_numpy(d_np))
            I.copy_(torch.from_numpy(i_np))
        if len(self.segments) > 1:
            I.copy_(self._to_global(I))
        if self._single():
            return D, I
        # THE exchange step of the path: one all-gather of nq*k*12 bytes per rank
        recv_flat = torch.empty(self.world * record, dtype=torch.uint8, device=q.device)
        if q.is_cuda and self.dist.get_backend(self.group) == "gloo":
            # rehearsal of the N > 1 path on a box without RCCL peers: gloo moves host memory
            host = torch.empty(self.world * record, dtype=torch.uint8)
            self.dist.all_gather_into_tensor(host, send.cpu(), group=self.group)
            recv_flat.copy_(host)
        else:
            self.dist.all_gather_into_tensor(recv_flat, send, group=self.group)
        recv = recv_flat.view(self.world, record)
        if self._merge is None and q.is_cuda:
            return self._merge_packed_hip(recv, nq, k, record)
        if self._merge is None:
            raise RuntimeError("ShardedFlatIndex: the merge of the gathered top-k lists runs on the HIP device "
                               "(css_merge_topk_packed_dev); queries on the CPU need merge=<callable> (test doubles only)")
        Ig = recv[:, :ib].view(torch.int64).view(self.world, nq, k)
        Dg = recv[:, ib:db].view(torch.float32).view(self.world, nq, k)
        return self._merge(Dg.contiguous(), Ig.contiguous(), k)

    def search(self, q: np.ndarray, k: int, normalize: bool = False, allow=None):
        import torch

        qt = torch.from_numpy(self._queries(q))
        if self.device_index is not None and torch.cuda.is_available():
            qt = qt.to(f"cuda:{self.device_index}")
        D, I = self.search_tensors(qt, k, normalize, allow=allow)
        return D.cpu().numpy(), I.cpu().numpy()

    # -- range search ------------------------------------------------------------------------------------------
    def range_search(self, q, thresh: float, normalize: bool = False, allow=None):
        """``IndexFlat.range_search`` over the shards: ``(lims, D, I)`` with global ids on every rank, each query's hits
        best score first and equal scores by ascending id.  Every rank range-searches its shard (local allow-mask as in
        ``search_tensors``); the variable-length lists then take two collective steps -- one all-gather of the
        per-query counts, one of the payload (ids, scores) padded to the largest rank's size -- and every rank merges
        per query.  With one rank there is no exchange.  Results live on the host, as the local call returns them."""
        qa = self._queries(q)
        nq = qa.shape[0]
        lims, D, I = self.local.range_search(qa, thresh, normalize=normalize, allow=self._local_allow(allow))
        lims = np.asarray(lims, dtype=np.int64)
        D = np.asarray(D, dtype=np.float32)
        I = self._to_global_np(np.asarray(I, dtype=np.int64))
        if self._single() or nq == 0:   # (nq is the same on every rank)
            return lims, D, I
        # step 1: the per-query hit counts of every rank
        all_counts = self._all_gather_host(np.diff(lims))
        totals = all_counts.sum(axis=1)
        most = int(totals.max())
        if most == 0:
            return np.zeros(nq + 1, dtype=np.int64), np.empty(0, np.float32), np.empty(0, np.int64)
        # step 2: the payload, every rank's record padded to the largest one: [most int64 ids][most float32 scores]
        record = (12 * most + 15) // 16 * 16
        send = np.zeros(record, dtype=np.uint8)
        send[:8 * I.shape[0]] = I.view(np.uint8)
        send[8 * most:8 * most + 4 * D.shape[0]] = D.view(np.uint8)
        recv = self._all_gather_host(send)
        ids, scores, qid = [], [], []
        for r in range(self.world):
            t = int(totals[r])
            ids.append(recv[r, :8 * t].view(np.int64))
            scores.append(recv[r, 8 * most:8 * most + 4 * t].view(np.float32))
            qid.append(np.repeat(np.arange(nq, dtype=np.int64), all_counts[r]))
        ids, scores, qid = np.concatenate(ids), np.concatenate(scores), np.concatenate(qid)
        # per-query merge: query, then best score first (IP descending, L2 ascending), then ascending id
        order = self._best_first(scores, ids, qid)
        out_lims = np.zeros(nq + 1, dtype=np.int64)
        np.cumsum(all_counts.sum(axis=0), out=out_lims[1:])
        return out_lims, np.ascontiguousarray(scores[order]), np.ascontiguousarray(ids[order])

    # -- facet counts ------------------------------------------------------------------------------------------
    def facets(self, q, thresh: float, buckets=None, nbuckets: Optional[int] = None, normalize: bool = False, allow=None,
               by_attribute: Optional[int] = None):
        """``IndexFlat.facets`` over the shards (collective: every rank passes the same arguments): a ``FacetCounts``
        with global ids on every rank.  ``buckets`` and ``allow`` are in GLOBAL numbering and are cut per shard through
        the segment table, as ``set_groups`` and ``_local_allow`` do (``buckets=None``: the labels ``set_groups``
        stored); tombstones are left out.  Every rank counts its shard, then ONE sum all-reduce adds
        ``counts | total | unbucketed`` (int64) and ONE all-gather moves every rank's ``(best_score, best global id)``
        per entry, merged by best score, then smaller global id.  A row's score is its own fp32 chain wherever it lies
        and counts are integers, so the result equals the unsharded one byte for byte.  With one rank there is no
        exchange.  ``by_attribute=slot``: the buckets are the int32 attribute column ``set_attribute`` stored on every
        shard (``nbuckets`` required, ``buckets`` must be ``None``)."""
        from .flat_index import ATTR_I32, FacetCounts, attr_slot, facet_args

        qa = self._queries(q)
        more = {}
        if by_attribute is not None:
            slot = attr_slot(by_attribute, "facets")
            if buckets is not None:
                raise ValueError("facets: give buckets or by_attribute, not both")
            if nbuckets is None:
                raise ValueError("facets: nbuckets is required with by_attribute")
            typ = self._attr_types.get(slot, -1)
            if typ != ATTR_I32:
                raise ValueError(f"facets: attribute slot {slot} " + ("was never set" if typ < 0 else "holds float32 values"))
            if self.shard_sizes[self.rank]:   # (a shard without rows has no column, and no hit either)
                more["by_attribute"] = slot
        thresh, b, nb = facet_args(thresh, buckets, nbuckets, self.ntotal_global)
        loc = self.local.facets(qa, thresh, buckets=None if b is None else self.local_rows_of(b), nbuckets=nb,
                                normalize=normalize, allow=self._local_allow(allow), **more)
        counts, total, unb = (np.ascontiguousarray(a, dtype=np.int64) for a in (loc.counts, loc.total, loc.unbucketed))
        S = np.ascontiguousarray(loc.best_score, dtype=np.float32)
        I = np.ascontiguousarray(self._to_global_np(np.asarray(loc.best_id, dtype=np.int64)))
        if self._single() or qa.shape[0] == 0:
            return FacetCounts(counts, S, I, total, unb)
        n, nq = counts.size, qa.shape[0]
        sums = self._sum_over_ranks(np.concatenate([counts.reshape(-1), total, unb]))
        send = np.empty(12 * n, dtype=np.uint8)   # [n int64 ids][n float32 scores]
        send[:8 * n] = I.reshape(-1).view(np.uint8)
        send[8 * n:] = S.reshape(-1).view(np.uint8)
        recv = self._all_gather_host(send)
        Ig = np.stack([recv[r, :8 * n].view(np.int64) for r in range(self.world)], axis=1)      # [n, world]
        Sg = np.stack([recv[r, 8 * n:].view(np.float32) for r in range(self.world)], axis=1)
        # per entry: the shards that have a hit first, then best score (IP descending, L2 ascending), then smaller id
        first = np.lexsort((Ig, -Sg if self.metric == 0 else Sg, Ig < 0), axis=1)[:, :1]
        return FacetCounts(np.ascontiguousarray(sums[:n].reshape(nq, nb)),
                           np.ascontiguousarray(np.take_along_axis(Sg, first, axis=1).reshape(nq, nb)),
                           np.ascontiguousarray(np.take_along_axis(Ig, first, axis=1).reshape(nq, nb)),
                           np.ascontiguousarray(sums[n:n + nq]), np.ascontiguousarray(sums[n + nq:]))

    # -- attribute columns and filters -------------------------------------------------------------------------
    def set_attribute(self, slot: int, global_values, row0: int = 0) -> None:
        """``IndexFlat.set_attribute`` in GLOBAL numbering (collective: every rank passes the same values): values of the
        global rows ``[row0, row0 + len(global_values))``; every rank writes the part its shard holds, through the
        segment table like ``set_groups``.  The slot has ONE type on all shards: a shard none of whose rows were in the
        range still gets the (all-default) column, so that a later ``where`` finds the slot on every rank."""
        from .flat_index import ATTR_F32, attr_slot, attr_values

        slot = attr_slot(slot)
        v, typ = attr_values(global_values)
        row0 = int(row0)
        self._check_rows("set_attribute", row0, v.shape[0])
        have = self._attr_types.get(slot, -1)
        if have >= 0 and have != typ:
            raise ValueError(f"set_attribute: attribute slot {slot} holds {'float32' if have == ATTR_F32 else 'int32'} values")
        if v.shape[0] == 0:
            return
        self._attr_types[slot] = typ
        for l0, g0, n in self._overlaps(row0, v.shape[0]):
            self.local.set_attribute(slot, v[g0 - row0:g0 - row0 + n], row0=l0)
        if self.shard_sizes[self.rank] and self.local.attribute_type(slot) < 0:
            self.local.set_attribute(slot, np.full(1, np.nan, np.float32) if typ == ATTR_F32 else np.full(1, -1, np.int32))

    def get_attribute(self, slot: int) -> np.ndarray:
        """This shard's values of attribute ``slot`` in LOCAL row order (``local_rows_of`` of the global column)."""
        return self.local.get_attribute(slot)

    def attribute_type(self, slot: int) -> int:
        from .flat_index import attr_slot

        return self._attr_types.get(attr_slot(slot, "attribute_type"), -1)

    def drop_attribute(self, slot: int) -> None:
        from .flat_index import attr_slot

        if self._attr_types.pop(attr_slot(slot, "drop_attribute"), None) is not None:
            self.local.drop_attribute(slot)

    def where(self, clauses, allow=None, return_count: bool = False):
        """``IndexFlat.where`` over the shards (collective with ``return_count``): the boolean mask over THIS shard's
        rows in local order -- ``local_rows_of`` of the mask one index holding all rows would answer; ``allow`` is in
        GLOBAL numbering and the tombstones are left out, as in every search.  ``return_count=True`` returns
        ``(local mask, number of rows that pass on ALL shards)``: ONE sum all-reduce of an int64."""
        from .flat_index import where_args

        where_args(clauses, self.attribute_type)   # the same refusal on every rank, before any shard is asked
        la = self._local_allow(allow)
        if self.shard_sizes[self.rank]:
            mask, count = self.local.where(clauses, allow=la, return_count=True)
        else:
            mask, count = np.zeros(0, dtype=np.bool_), 0
        if not return_count:
            return mask
        return mask, int(self._sum_over_ranks(np.array([count], dtype=np.int64))[0])

    # -- grouped search ----------------------------------------------------------------------------------------
    def set_groups(self, global_labels, row0: int = 0) -> None:
        """``IndexFlat.set_groups`` in GLOBAL numbering (collective: every rank passes the same labels): labels of the
        global rows ``[row0, row0 + len(global_labels))``; every rank writes the part its shard holds, through the
        segment table like ``local_rows_of``.  A label means the same group on every shard."""
        from .flat_index import labels_as_int32

        g = labels_as_int32(global_labels)
        row0 = int(row0)
        self._check_rows("set_groups", row0, g.shape[0])
        for l0, g0, n in self._overlaps(row0, g.shape[0]):
            self.local.set_groups(g[g0 - row0:g0 - row0 + n], row0=l0)

    def search_grouped(self, q, k: int, normalize: bool = False, allow=None):
        """``IndexFlat.search_grouped`` over the shards: ``(D, I, G)`` with global ids on every rank.  Every rank runs
        the grouped search of its shard (local allow-mask as in ``search_tensors``), maps its ids to global, and ONE
        all-gather moves the ``nq * k`` (id, score, label) records of every rank; every rank then merges per query on
        the host: sort by (score, id), then ``flat_index.collapse_groups``.  Exact: a group of the global top-k is
        among the top-k groups of the shard that holds its best row, because every group ranked above it on that
        shard also ranks above it globally.  With one rank there is no exchange."""
        from .flat_index import MAX_GROUP_K, collapse_groups

        qa, k = self._queries(q), int(k)
        if k < 1 or k > MAX_GROUP_K:
            raise ValueError(f"k={k} outside [1, {MAX_GROUP_K}]")
        D, I, G = self.local.search_grouped(qa, k, normalize=normalize, allow=self._local_allow(allow))
        I, (D, G), local = self._columns(I, (D, G), last=np.int32)   # 16-byte (id, score, label) records
        return (D, I, G) if local else collapse_groups(D, I, G, k, self.metric)

    # -- prior-weighted search ---------------------------------------------------------------------------------
    def set_priors(self, global_priors, row0: int = 0) -> None:
        """``IndexFlat.set_priors`` in GLOBAL numbering (collective: every rank passes the same priors): priors of the
        global rows ``[row0, row0 + len(global_priors))``; every rank writes the part its shard holds, through the
        segment table like ``set_groups``."""
        from .flat_index import priors_as_f32

        p = priors_as_f32(global_priors)
        row0 = int(row0)
        self._check_rows("set_priors", row0, p.shape[0])
        for l0, g0, n in self._overlaps(row0, p.shape[0]):
            self.local.set_priors(p[g0 - row0:g0 - row0 + n], row0=l0)

    def search_prior(self, q, k: int, weight: float, normalize: bool = False, allow=None):
        """``IndexFlat.search_prior`` over the shards: ``(D, I, S)`` with global ids on every rank.  Every rank runs the
        prior-weighted search of its shard (local allow-mask as in ``search_tensors``), maps its ids to global, and ONE
        all-gather moves the ``nq * k`` (id, fused value, raw score) records of every rank; every rank then sorts per
        query by (fused value, id) and keeps the first ``k``.  Exact: a row of the global top-k is in the top-k of its
        shard.  With one rank there is no exchange."""
        from .flat_index import MAX_PRIOR_K

        qa, k, weight = self._queries(q), int(k), float(weight)
        if k < 1 or k > MAX_PRIOR_K:
            raise ValueError(f"k={k} outside [1, {MAX_PRIOR_K}]")
        if not np.isfinite(weight):
            raise ValueError(f"weight={weight} is not finite")
        D, I, S = self.local.search_prior(qa, k, weight, normalize=normalize, allow=self._local_allow(allow))
        I, (D, S), _ = self._columns(I, (D, S))   # 16-byte (id, fused value, raw score) records
        return tuple(np.ascontiguousarray(a[..., :k]) for a in (D, I, S))

    # -- search by examples ------------------------------------------------------------------------------------
    def _local_ids(self, global_ids: np.ndarray) -> np.ndarray:
        """Global ids -> local row numbers through the segment table (one rank: every id is owned)."""
        out = np.full(global_ids.shape, -1, dtype=np.int64)
        for l0, g0, n in self.segments:
            own = (global_ids >= g0) & (global_ids < g0 + n)
            out[own] = global_ids[own] - g0 + l0
        return out

    def search_examples(self, pos=None, neg=None, pos_ids=(), neg_ids=(), k: int = 10, gamma: float = 0.5,
                        normalize: bool = False, exclude_ids: bool = True, allow=None):
        """``IndexFlat.search_examples`` over the shards (collective: every rank passes the same arguments):
        ``(D[k], I[k], S[k])`` with global ids on every rank; ``pos_ids`` / ``neg_ids`` are GLOBAL row ids.  The id
        examples become vectors by the all-reduce of ``search_by_ids`` (the owning shard supplies the stored row), the
        vector examples are normalised on the host where ``normalize`` is set, and every rank runs the local call for
        ``k + nids`` rows with EVERY example passed as a vector and nothing excluded.  ONE all-gather moves the 16-byte
        ``[id | D | S]`` records; every rank sorts by ``(D, id)``, drops the example ids (``exclude_ids``) and keeps
        ``k``.  Exact: a row of the global answer is among the best ``k + nids`` of its shard.  ``k + nids <= 128``.
        The host normalisation divides in float32 like the device does but sums the squares in another order, so
        with ``normalize`` the last bits of ``D`` and ``S`` can differ from the single index.  With one rank the whole
        call is the local one, ids and exclusion on the device.  An id outside ``[0, ntotal_global)`` raises
        ``ValueError`` on every rank, before any collective."""
        from .flat_index import MAX_EXAMPLES_K, example_args, example_vectors, ids_as_int64

        what = "search_examples"
        vp, vn = example_vectors(pos, self.d, what), example_vectors(neg, self.d, what)
        ip, ineg = ids_as_int64(pos_ids, what), ids_as_int64(neg_ids, what)
        nids = ip.shape[0] + ineg.shape[0]
        k, gamma = example_args(k, gamma, vp.shape[0] + ip.shape[0], vp.shape[0] + vn.shape[0] + nids)
        ids = np.concatenate([ip, ineg])
        self._check_ids(what, ids)
        if self._single():
            D, I, S = self.local.search_examples(vp, vn, self._local_ids(ip), self._local_ids(ineg), k=k, gamma=gamma,
                                                 normalize=normalize, exclude_ids=exclude_ids,
                                                 allow=self._local_allow(allow))
            return D, np.ascontiguousarray(self._to_global_np(I)), S
        drop = ids if exclude_ids else ids[:0]
        kk = k + drop.shape[0]
        if kk > MAX_EXAMPLES_K:
            raise ValueError(f"search_examples: k + id examples = {kk} beyond {MAX_EXAMPLES_K}")
        if normalize:
            unit = lambda v: (v / (np.sqrt((v * v).sum(axis=1, dtype=np.float32, keepdims=True))
                                   + np.float32(1e-8))).astype(np.float32)
            vp, vn = unit(vp), unit(vn)
        rows = self._owned_rows(ids)
        D, I, S = self.local.search_examples(np.concatenate([vp, rows[:ip.shape[0]]]), np.concatenate([vn, rows[ip.shape[0]:]]),
                                             k=kk, gamma=gamma, normalize=False, exclude_ids=False,
                                             allow=self._local_allow(allow))
        I, (D, S), _ = self._columns(I, (D, S))   # 16-byte (id, D, S) records
        keep = np.flatnonzero(~np.isin(I[0], drop))[:k]
        return D[0][keep], I[0][keep], S[0][keep]

    # -- term lists and hybrid search --------------------------------------------------------------------------
    def set_terms(self, lists, row0: Optional[int] = None) -> None:
        """``IndexFlat.set_terms`` in GLOBAL numbering (collective: every rank passes the same lists): the term lists
        of the global rows ``[row0, row0 + n)``; ``row0 = None`` appends after the global rows that have lists, a lower
        ``row0`` first drops the lists of all global rows ``>= row0``.  Every rank writes the part its shard holds
        through the segment table.  Local order is global order within a shard, so the local lists stay append-only:
        the shard's rows of the call are consecutive local rows that start at its first local row ``>= row0``."""
        from .lexical import lists_as_csr

        off, tok = lists_as_csr(lists)
        n = off.shape[0] - 1
        row0 = self._terms_global if row0 is None else int(row0)
        self._check_rows("set_terms", row0, n)
        if row0 > self._terms_global:
            raise ValueError(f"set_terms: row0={row0} beyond the {self._terms_global} rows that have lists (lists are append-only)")
        if n == 0 and row0 == self._terms_global:
            return
        local_row0, loff, (ltok,) = self._local_csr(row0, off, (tok,))
        self.local.set_terms((loff, ltok), row0=local_row0)
        self._terms_global = row0 + n

    def _local_csr(self, row0: int, off: np.ndarray, values):
        """This shard's part of per-row lists in CSR form over the GLOBAL rows ``[row0, row0 + n)``: ``(the first local
        row >= global row0, local offsets from 0, the entries of each array of values)``, through the segment table."""
        n = off.shape[0] - 1
        local_row0 = sum(min(max(row0 - g0, 0), m) for _, g0, m in self.segments)   # local rows below global row0
        parts_off, parts, count = [np.zeros(1, np.int64)], [[] for _ in values], 0
        for _, lo, m in self._overlaps(row0, n):
            a, e = int(off[lo - row0]), int(off[lo - row0 + m])
            parts_off.append(off[lo - row0 + 1:lo - row0 + m + 1] - a + count)
            count += e - a
            for p, v in zip(parts, values):
                p.append(v[a:e])
        loff = np.concatenate(parts_off).astype(np.int64)
        return local_row0, loff, tuple(np.concatenate(p) if p else v[:0] for p, v in zip(parts, values))

    def term_stats(self, terms):
        """``IndexFlat.term_stats`` over the shards (collective): ``(df, ndocs, total_len)`` of the whole index -- the
        integer sums of the shards' statistics."""
        t = np.asarray(terms, dtype=np.int64).reshape(-1)
        df, _, total = self.local.term_stats(t)
        both = self._sum_over_ranks(np.concatenate([np.asarray(df, np.int64), np.array([total], np.int64)]))
        return both[:-1].copy(), int(self.ntotal_global), int(both[-1])

    def search_hybrid(self, q, terms, weights, k: int, alpha: float, k1: float = 1.2, b: float = 0.75,
                      avgdl: Optional[float] = None, normalize: bool = False, allow=None):
        """``IndexFlat.search_hybrid`` over the shards (collective): ``(D, I, S, L)`` with global ids on every rank.
        Every shard scores with the CALLER's weights and constants (``avgdl=None``: the global statistics), so a row's
        values do not depend on the shard that holds it and the merged result equals the unsharded one bit for bit.
        The exchange moves 20-byte records (id, D, S, L); every rank keeps the first ``k`` by ``(D, id)``."""
        from .flat_index import hybrid_args

        qa = self._queries(q)
        if qa.shape[0] != 1:
            raise ValueError(f"search_hybrid: one query per call, got {qa.shape[0]}")
        t, w, k, alpha, k1, b, avgdl = hybrid_args(terms, weights, k, alpha, k1, b, avgdl)
        if avgdl is None:
            _, ndocs, total = self.term_stats(())
            avgdl = total / ndocs if ndocs > 0 and total > 0 else 1.0
        D, I, S, L = self.local.search_hybrid(qa, t, w, k, alpha, k1=k1, b=b, avgdl=avgdl, normalize=normalize,
                                              allow=self._local_allow(allow))
        I, (D, S, L), _ = self._columns(I, (D, S, L))
        return tuple(np.ascontiguousarray(a[..., :k]) for a in (D, I, S, L))

    # -- sparse vectors and sparse search ----------------------------------------------------------------------
    def set_sparse(self, vectors, row0: Optional[int] = None) -> None:
        """``IndexFlat.set_sparse`` in GLOBAL numbering (collective: every rank passes the same vectors; no
        communication): the sparse vectors of the global rows ``[row0, row0 + n)``, append-only like ``set_terms`` and
        routed through the segment table the same way."""
        from .flat_index import sparse_as_csr

        off, t, w = sparse_as_csr(vectors)
        n = off.shape[0] - 1
        row0 = self._sparse_global if row0 is None else int(row0)
        self._check_rows("set_sparse", row0, n)
        if row0 > self._sparse_global:
            raise ValueError(f"set_sparse: row0={row0} beyond the {self._sparse_global} rows that have vectors (vectors are append-only)")
        if n == 0 and row0 == self._sparse_global:
            return
        local_row0, loff, (lt, lw) = self._local_csr(row0, off, (t, w))
        self.local.set_sparse((loff, lt, lw), row0=local_row0)
        self._sparse_global = row0 + n

    @property
    def sparse_rows(self) -> int:
        """The leading GLOBAL rows that have sparse vectors."""
        return self._sparse_global

    def search_sparse(self, terms, weights, k: int, allow=None):
        """``IndexFlat.search_sparse`` over the shards (collective): ``(D, I)`` with global ids on every rank.  A row's
        dot product is a function of its own vector and the query, with no corpus statistics, so the merged result
        equals the single index's in bytes.  The exchange moves 12-byte records (id, D); every rank keeps the first
        ``k`` by ``(D descending, id)`` on an index of either metric."""
        from .flat_index import sparse_args

        t, w, k, _ = sparse_args(terms, weights, k)
        D, I = self.local.search_sparse(t, w, k, allow=self._local_allow(allow))
        I, (D,), _ = self._columns(I, (D,), metric=0)
        return tuple(np.ascontiguousarray(a[..., :k]) for a in (D, I))

    def search_hybrid_sparse(self, q, terms, weights, k: int, alpha: float, normalize: bool = False, allow=None):
        """``IndexFlat.search_hybrid_sparse`` over the shards (collective): ``(D, I, S, L)`` with global ids on every
        rank, the exchange and the merge of ``search_hybrid``."""
        from .flat_index import sparse_args

        qa = self._queries(q)
        if qa.shape[0] != 1:
            raise ValueError(f"search_hybrid_sparse: one query per call, got {qa.shape[0]}")
        t, w, k, alpha = sparse_args(terms, weights, k, alpha, what="search_hybrid_sparse")
        D, I, S, L = self.local.search_hybrid_sparse(qa, t, w, k, alpha, normalize=normalize, allow=self._local_allow(allow))
        I, (D, S, L), _ = self._columns(I, (D, S, L))
        return tuple(np.ascontiguousarray(a[..., :k]) for a in (D, I, S, L))

    # -- token matrices and MaxSim search ------------------------------------------------------------------------
    def set_tokens(self, mats, keep=None, row0: Optional[int] = None) -> None:
        """``IndexFlat.set_tokens`` in GLOBAL numbering (collective: every rank passes the same matrices; no
        communication): the token matrices of the global rows ``[row0, row0 + n)``, append-only like ``set_sparse`` and
        routed through the segment table the same way."""
        from .flat_index import tokens_as_csr

        off, tok, P = tokens_as_csr(mats, keep)
        n = off.shape[0] - 1
        row0 = self._tokens_global if row0 is None else int(row0)
        self._check_rows("set_tokens", row0, n)
        if row0 > self._tokens_global:
            raise ValueError(f"set_tokens: row0={row0} beyond the {self._tokens_global} rows that have matrices (matrices are append-only)")
        if self._tokens_global and row0 and n and P != self._token_dim:
            raise ValueError(f"set_tokens: P={P}, but the stored matrices have P={self._token_dim} (only a rewrite from row 0 changes it)")
        if n == 0 and row0 == self._tokens_global:
            return
        local_row0, loff, (ltok,) = self._local_csr(row0, off, (tok,))
        self.local.set_tokens((loff, ltok, P), row0=local_row0)
        self._tokens_global, self._token_dim = row0 + n, P if n else self._token_dim

    @property
    def token_rows(self) -> int:
        """The leading GLOBAL rows that have token matrices."""
        return self._tokens_global

    @property
    def token_dim(self) -> int:
        """The width P of the stored token vectors (0: no row has a matrix)."""
        return self._token_dim if self._tokens_global else 0

    def drop_tokens(self) -> None:
        """``IndexFlat.drop_tokens`` on every shard (collective; no communication)."""
        self.local.drop_tokens()
        self._tokens_global, self._token_dim = 0, 0

    def get_tokens(self, row0: int = 0, n: Optional[int] = None):
        """``IndexFlat.get_tokens`` of the GLOBAL rows ``[row0, row0 + n)`` on every rank (collective): the shard that
        owns a row supplies its length and its tokens, every other shard zeros, in two ``_sum_over_ranks`` (exact: one
        contribution per entry)."""
        row0 = int(row0)
        n = self.ntotal_global - row0 if n is None else int(n)
        self._check_rows("get_tokens", row0, n)
        P = self.token_dim
        parts = [(lo - row0, m) + tuple(self.local.get_tokens(l0, m)) for l0, lo, m in self._overlaps(row0, n)] if P else []
        lens = np.zeros(n, dtype=np.int64)
        for at, m, loff, _ in parts:
            lens[at:at + m] = np.diff(loff)
        lens = self._sum_over_ranks(lens)
        off = np.zeros(n + 1, dtype=np.int64)
        np.cumsum(lens, out=off[1:])
        tok = np.zeros((int(off[-1]), max(P, 1)), dtype=np.int32)
        for at, m, _, ltok in parts:
            tok[off[at]:off[at + m]] = np.asarray(ltok).reshape(-1, P)   # (a shard without matrices gives [0, 0])
        return off, self._sum_over_ranks(tok).astype(np.uint16).reshape(int(off[-1]), P)

    # -- compressed token matrices ---------------------------------------------------------------------------------
    def set_token_codec(self, codec) -> None:
        """``IndexFlat.set_token_codec`` on every shard (collective: every rank passes the same codec; no
        communication).  A row's codes and score depend on its own matrix, the codec and the query alone, so the sharded
        results equal the single index's in bytes."""
        self.local.set_token_codec(codec)

    @property
    def token_codec_bits(self) -> int:
        return self.local.token_codec_bits

    def get_token_codec(self):
        return self.local.get_token_codec()

    def set_token_codes(self, offsets, codes, res, row0: Optional[int] = None) -> None:
        """``IndexFlat.set_token_codes`` in GLOBAL numbering (collective: every rank passes the same codes), routed
        through the segment table like ``set_tokens``."""
        from .flat_index import token_codes_as_csr

        codec = self.get_token_codec()
        if codec is None:
            raise ValueError("set_token_codes: the index has no token codec")
        off, codes, res = token_codes_as_csr(offsets, codes, res, codec)
        n = off.shape[0] - 1
        row0 = self._tokens_global if row0 is None else int(row0)
        self._check_rows("set_token_codes", row0, n)
        if row0 > self._tokens_global:
            raise ValueError(f"set_token_codes: row0={row0} beyond the {self._tokens_global} rows that have matrices (matrices are append-only)")
        if n == 0 and row0 == self._tokens_global:
            return
        local_row0, loff, (lcodes, lres) = self._local_csr(row0, off, (codes, res))
        self.local.set_token_codes(loff, lcodes, lres, row0=local_row0)
        self._tokens_global, self._token_dim = row0 + n, codec.P if n else self._token_dim

    def get_token_codes(self, row0: int = 0, n: Optional[int] = None):
        """``IndexFlat.get_token_codes`` of the GLOBAL rows ``[row0, row0 + n)`` on every rank (collective): summed over
        the ranks as ``get_tokens`` is (exact: one contribution per entry)."""
        codec = self.get_token_codec()
        if codec is None:
            raise ValueError("get_token_codes: the index has no token codec")
        row0 = int(row0)
        n = self.ntotal_global - row0 if n is None else int(n)
        self._check_rows("get_token_codes", row0, n)
        parts = [(lo - row0, m) + tuple(self.local.get_token_codes(l0, m)) for l0, lo, m in self._overlaps(row0, n)]
        lens = np.zeros(n, dtype=np.int64)
        for at, m, loff, _, _ in parts:
            lens[at:at + m] = np.diff(loff)
        lens = self._sum_over_ranks(lens)
        off = np.zeros(n + 1, dtype=np.int64)
        np.cumsum(lens, out=off[1:])
        both = np.zeros((int(off[-1]), 1 + codec.res_bytes), dtype=np.int32)   # [code | packed buckets] per token
        for at, m, _, lcodes, lres in parts:
            both[off[at]:off[at + m], 0] = lcodes
            both[off[at]:off[at + m], 1:] = lres
        both = self._sum_over_ranks(both)
        return off, both[:, 0].astype(np.uint16), np.ascontiguousarray(both[:, 1:].astype(np.uint8))

    def search_maxsim(self, q_mat, k: int, allow=None):
        """``IndexFlat.search_maxsim`` over the shards (collective): ``(D, I)`` with global ids on every rank.  A row's
        score is a function of its own matrix and the query, so the merged result equals the single index's in bytes.
        The exchange moves 12-byte records (id, D); every rank keeps the first ``k`` by ``(D descending, id)`` on an
        index of either metric."""
        from .flat_index import maxsim_args

        q, k, _ = maxsim_args(q_mat, k)
        D, I = self.local.search_maxsim(q, k, allow=self._local_allow(allow))
        I, (D,), _ = self._columns(I, (D,), metric=0)
        return tuple(np.ascontiguousarray(a[..., :k]) for a in (D, I))

    def search_maxsim_batch(self, q_mats, k: int, allow=None):
        """``IndexFlat.search_maxsim_batch`` over the shards (collective): ``(D [nq, k], I [nq, k])`` with global ids on
        every rank, row ``b`` the bytes of ``search_maxsim(q_mats[b], k, allow)``: the local batch call, then the column
        exchange of ``search_maxsim`` for all queries at once."""
        from .flat_index import maxsim_batch_args

        off, tok, k = maxsim_batch_args(q_mats, k)
        D, I = self.local.search_maxsim_batch([tok[off[b]:off[b + 1]] for b in range(off.shape[0] - 1)], k,
                                              allow=self._local_allow(allow))
        I, (D,), _ = self._columns(I, (D,), metric=0)
        return tuple(np.ascontiguousarray(a[..., :k]) for a in (D, I))

    def maxsim_ids(self, q_mat, ids) -> np.ndarray:
        """``IndexFlat.maxsim_ids`` of GLOBAL ``ids`` on every rank (collective): every id is routed to the shard that
        owns it through the segment table, the other shards contribute zero bits, then ONE ``_sum_over_ranks`` of the
        float32 bit patterns (exact: one contribution per id)."""
        from .flat_index import maxsim_args

        q, _, ids = maxsim_args(q_mat, ids=ids, what="maxsim_ids")
        self._check_ids("maxsim_ids", ids)
        out = np.zeros(ids.shape[0], dtype=np.float32)
        loc = self._local_ids(ids)
        own = np.flatnonzero(loc >= 0)
        if own.size:
            # (one segment: the local index adds id_base itself, so it is asked by global id)
            out[own] = self.local.maxsim_ids(q, ids[own] if len(self.segments) == 1 else loc[own])
        return self._sum_over_ranks(out.view(np.int32)).view(np.float32)

    def _max_over_ranks(self, a: np.ndarray) -> np.ndarray:
        """ONE max all-reduce of a host array (none with one rank, or for nothing)."""
        import torch

        if self.world == 1 or a.size == 0:
            return a
        t = torch.from_numpy(a).to(self._exchange_device())
        self.dist.all_reduce(t, op=self.dist.ReduceOp.MAX, group=self.group)
        return t.cpu().numpy()

    def maxsim_ids_batch(self, q_mats, ids) -> np.ndarray:
        """``IndexFlat.maxsim_ids_batch`` of GLOBAL ``ids [nq, f]`` on every rank (collective): every rank scores its
        own share with ONE local call (the ids of other shards name no row there: ``-inf``), then ONE max all-reduce
        of the ``[nq, f]`` scores (exact: one contribution per id that is not ``-inf``)."""
        from .flat_index import rerank_args

        _, off, tok, _, _, _, ids = rerank_args(None, q_mats, None, None, ids=ids, what="maxsim_ids_batch")
        mats = [tok[off[b]:off[b + 1]] for b in range(off.shape[0] - 1)]
        # (one segment: the local index adds id_base itself, so it is asked by global id)
        mine = np.where(self._local_ids(ids) >= 0, ids, -1) if len(self.segments) == 1 else self._local_ids(ids)
        out = np.full(ids.shape, -np.inf, dtype=np.float32)
        if (mine >= 0).any():
            out = np.ascontiguousarray(self.local.maxsim_ids_batch(mats, mine), dtype=np.float32)
        return self._max_over_ranks(out)

    def search_rerank_maxsim(self, q, q_mats, k: int, fetch: int, normalize: bool = False, floor=None, allow=None):
        """``IndexFlat.search_rerank_maxsim`` over the shards (collective): ``(D, I, S, R)`` with global ids on every
        rank, the single index's bytes.  The sharded ``search`` gives every rank the GLOBAL pool, every rank scores
        its own share of it (``maxsim_ids_batch``: one max all-reduce of ``[nq, fetch]`` scores), and every rank then
        ranks with the stable sort of ``search_rerank_maxsim_numpy``."""
        from .flat_index import rerank_args, search_rerank_maxsim_numpy

        a, off, tok, k, fetch, floor, _ = rerank_args(q, q_mats, k, fetch, floor, d=self.d)
        mats = [tok[off[b]:off[b + 1]] for b in range(off.shape[0] - 1)]
        if self._single():
            D, I, S, R = self.local.search_rerank_maxsim(a, mats, k, fetch, normalize=normalize, floor=floor,
                                                         allow=self._local_allow(allow))
            return D, np.ascontiguousarray(self._to_global_np(np.asarray(I, dtype=np.int64))), S, R
        S0, I0 = self.search(a, fetch, normalize, allow=allow)
        late = self.maxsim_ids_batch(mats, I0)
        return search_rerank_maxsim_numpy(S0, I0, late, k, floor)

    def maxsim_candidates(self, q_mat, ncand: int, allow=None):
        """``IndexFlat.maxsim_candidates`` over the shards (collective): ``(ids, approx)`` with global ids, ascending,
        on every rank.  A row's approximate score is a function of its own codes, the codec and the query, and a
        shard's best ``ncand`` hold its share of the global best ``ncand``: ONE all-gather of every rank's
        ``[count | ids | approx]`` record, then every rank keeps the first ``ncand`` of ``lexsort((id, -approx))`` --
        the single index's bytes."""
        from .flat_index import maxsim_args, prune_args

        q, _, _ = maxsim_args(q_mat, what="maxsim_candidates")
        _, ncand = prune_args(None, ncand, "maxsim_candidates")
        ids, approx = self.local.maxsim_candidates(q, ncand, allow=self._local_allow(allow))
        ids = np.ascontiguousarray(self._to_global_np(np.asarray(ids, dtype=np.int64)))
        approx = np.ascontiguousarray(approx, dtype=np.float32)
        if self._single():
            return ids, approx
        n = ids.shape[0]
        send = np.zeros(8 + 12 * ncand, dtype=np.uint8)
        send[:8] = np.array([n], dtype=np.int64).view(np.uint8)
        send[8:8 + 8 * n] = ids.view(np.uint8)
        send[8 + 8 * ncand:8 + 8 * ncand + 4 * n] = approx.view(np.uint8)
        recv = self._all_gather_host(send)
        counts = [int(recv[r, :8].view(np.int64)[0]) for r in range(self.world)]
        ids = np.concatenate([recv[r, 8:8 + 8 * c].view(np.int64) for r, c in enumerate(counts)])
        approx = np.concatenate([recv[r, 8 + 8 * ncand:8 + 8 * ncand + 4 * c].view(np.float32) for r, c in enumerate(counts)])
        take = np.lexsort((ids, -(approx + np.float32(0.0))))[:ncand]
        take = take[np.argsort(ids[take], kind="stable")]
        return np.ascontiguousarray(ids[take]), np.ascontiguousarray(approx[take])

    def search_maxsim_pruned(self, q_mat, k: int, ncand: int, allow=None):
        """``IndexFlat.search_maxsim_pruned`` over the shards (collective): ``(D, I)`` with global ids on every rank,
        the single index's bytes.  Every rank forms the GLOBAL candidates (``maxsim_candidates``), scores its own
        share exactly with ``maxsim_ids``, keeps its best ``k`` by ``(score descending, id)``, and the column exchange
        of ``search_maxsim`` ranks the result."""
        from .flat_index import maxsim_args, prune_args

        q, _, _ = maxsim_args(q_mat, what="search_maxsim_pruned")
        k, ncand = prune_args(k, ncand)
        if self._single():
            D, I = self.local.search_maxsim_pruned(q, k, ncand, allow=self._local_allow(allow))
            return np.ascontiguousarray(D), np.ascontiguousarray(self._to_global_np(np.asarray(I, dtype=np.int64)))
        ids, _ = self.maxsim_candidates(q, ncand, allow=allow)
        loc = self._local_ids(ids)
        own = np.flatnonzero(loc >= 0)
        # (one segment: the local index adds id_base itself, so it is asked by global id and answers with it)
        mine = ids[own] if len(self.segments) == 1 else loc[own]
        D = np.full((1, k), -np.finfo(np.float32).max, dtype=np.float32)
        I = np.full((1, k), -1, dtype=np.int64)
        if own.size:
            sc = np.asarray(self.local.maxsim_ids(q, mine), dtype=np.float32)
            order = np.lexsort((ids[own], -sc))[:k]
            D[0, :order.size], I[0, :order.size] = sc[order], mine[order]
        I, (D,), _ = self._columns(I, (D,), metric=0)
        return tuple(np.ascontiguousarray(a[..., :k]) for a in (D, I))

    # -- significant terms -------------------------------------------------------------------------------------
    def _exchange_counts(self, local_mask):
        """``(terms ascending, counts, rows)`` of the whole index for a mask over THIS shard's rows (``None``: every
        row): every shard's ``subset_terms`` added up by term, and the number of masked rows that have lists.  The
        variable-length pairs move the way ``range_search`` moves its hits: one all-gather of the sizes, one of the
        pairs padded to the largest shard's."""
        t_local = sum(min(max(self._terms_global - g0, 0), m) for _, g0, m in self.segments)   # local rows with lists
        rows = t_local if local_mask is None else int(np.count_nonzero(np.asarray(local_mask)[:t_local]))
        t, f = self.local.subset_terms(local_mask)
        t, f = np.ascontiguousarray(t, dtype=np.uint32), np.ascontiguousarray(f, dtype=np.int64)
        if self._single():
            return t, f, rows
        sizes = self._all_gather_host(np.array([t.shape[0], rows], dtype=np.int64))
        most, rows = int(sizes[:, 0].max()), int(sizes[:, 1].sum())
        if most == 0:
            return np.zeros(0, np.uint32), np.zeros(0, np.int64), rows
        record = (12 * most + 15) // 16 * 16   # [most int64 counts][most uint32 terms]
        send = np.zeros(record, dtype=np.uint8)
        send[:8 * f.shape[0]] = f.view(np.uint8)
        send[8 * most:8 * most + 4 * t.shape[0]] = t.view(np.uint8)
        recv = self._all_gather_host(send)
        ts = np.concatenate([recv[r, 8 * most:8 * most + 4 * int(sizes[r, 0])].view(np.uint32) for r in range(self.world)])
        fs = np.concatenate([recv[r, :8 * int(sizes[r, 0])].view(np.int64) for r in range(self.world)])
        order = np.argsort(ts, kind="stable")
        ts, fs = ts[order], fs[order]
        first = np.flatnonzero(np.concatenate([[True], ts[1:] != ts[:-1]]))
        return np.ascontiguousarray(ts[first]), np.add.reduceat(fs, first).astype(np.int64), rows

    def subset_terms(self, allow=None):
        """``IndexFlat.subset_terms`` over the shards (collective; ``allow`` is a mask over the GLOBAL rows, tombstones
        are left out): the integer sums of the shards' counts, the same on every rank."""
        return self._exchange_counts(self._local_allow(allow))[:2]

    def significant_terms(self, allow=None, m: int = 20, min_count: int = 2, background=None):
        """``IndexFlat.significant_terms`` over the shards (collective; masks over the GLOBAL rows): the shards'
        ``subset_terms`` are exchanged and added by term, the background counts come from the sharded ``term_stats`` (or
        from a second exchange under a ``background`` mask), and ``lexical.significant_from_counts`` ranks -- integers
        in, so the result equals the unsharded one byte for byte."""
        from .lexical import significant_args, significant_from_counts

        m, min_count = significant_args(m, min_count)
        T = self._terms_global
        for mask in (allow, background):
            if mask is not None and np.asarray(mask).shape != (self.ntotal_global,):
                raise ValueError(f"mask has {np.asarray(mask).shape} entries, the sharded index {self.ntotal_global} rows")
        if background is not None:
            sel = np.ones(T, dtype=bool) if allow is None else np.asarray(allow, dtype=bool)[:T]
            bad = np.flatnonzero(sel & ~np.asarray(background, dtype=bool)[:T])
            if bad.size:
                raise ValueError(f"significant_terms: row {int(bad[0])} is selected but not in the background")
        t, f, FG = self._exchange_counts(self._local_allow(allow))
        if background is None:
            b, BG = np.asarray(self.term_stats(t)[0], dtype=np.int64), T
        else:
            bt, bc, BG = self._exchange_counts(self._local_allow(background))
            b = bc[np.searchsorted(bt, t)]   # (the selection lies within the background: every term is there)
        return significant_from_counts(t, f, b, FG, BG, m, min_count)

    # -- diversified search ------------------------------------------------------------------------------------
    def search_diverse(self, q, k: int, lam: float = 0.5, fetch: int = 0, normalize: bool = False, allow=None):
        """``IndexFlat.search_diverse`` over the shards (collective: every rank passes the same arguments): ``(D, I)``
        with global ids, in pick order, on every rank.  Three steps: (1) the usual search for ``fetch`` rows -- local
        masked search, the one packed all-gather, the merge -- after which every rank holds the global pool; (2) the
        rank that owns a candidate supplies its stored row, every other rank zeros, and ONE sum all-reduce of the
        ``[nq, fetch, d]`` buffer hands every rank every candidate's row (exact: one non-zero contribution per row, the
        trick of ``search_by_ids``); (3) ``flat_index.mmr_select`` runs on every rank.  The exchange of step 2 is
        ``nq * fetch * d * 4`` bytes (393 KB per query at ``fetch = 128``, ``d = 768``), so the call is meant for few
        queries -- the interactive search, not a batch job.  With one rank (and no forced exchange) the whole call is
        the local index's ``search_diverse``, selection on the device included."""
        from .flat_index import diverse_args, mmr_select

        qa = self._queries(q)
        k, fetch, lam = diverse_args(k, fetch, lam)
        if self._single():
            D, I = self.local.search_diverse(qa, k, lam=lam, fetch=fetch, normalize=normalize,
                                             allow=self._local_allow(allow))
            I = self._to_global_np(np.asarray(I, dtype=np.int64))
            return np.ascontiguousarray(D, dtype=np.float32), np.ascontiguousarray(I)
        if qa.shape[0] == 0:
            return np.empty((0, k), dtype=np.float32), np.empty((0, k), dtype=np.int64)
        S, I = self.search(qa, fetch, normalize=normalize, allow=allow)
        return mmr_select(S, I, self._owned_rows(I), k, lam, self.metric)

    # -- related rows ----------------------------------------------------------------------------------------------
    def search_by_ids(self, ids, k: int, exclude_self: bool = True, allow=None):
        """``IndexFlat.search_by_ids`` over the shards (collective: every rank passes the same arguments): ``ids`` are
        GLOBAL row ids.  The rank that owns an anchor supplies its stored row, every other rank zeros, and ONE sum
        all-reduce of the ``[nq, d]`` buffer hands every rank every query (exact: one non-zero contribution per row).
        Then the usual search runs for ``k + 1`` -- local masked search, one all-gather, merge -- and the anchor's
        global id is dropped after the merge (copies of the anchor on any shard stay).  An id outside
        ``[0, ntotal_global)`` raises ``ValueError`` on every rank, before any collective."""
        from .flat_index import MAX_K, drop_self, ids_as_int64

        a = ids_as_int64(ids)
        k = int(k)
        kmax = MAX_K - 1 if exclude_self else MAX_K
        if k < 1 or k > kmax:
            raise ValueError(f"k={k} outside [1, {kmax}]")
        self._check_ids("search_by_ids", a)
        if a.shape[0] == 0:
            return np.empty((0, k), dtype=np.float32), np.empty((0, k), dtype=np.int64)
        D, I = self.search(self._owned_rows(a), k + 1 if exclude_self else k, normalize=False, allow=allow)
        return drop_self(D, I, a) if exclude_self else (D, I)

    # -- rows back out (index files, compaction) ---------------------------------------------------------------
    def reconstruct_n(self, row0: int, n: int) -> np.ndarray:
        """Rows ``[row0, row0 + n)`` in GLOBAL numbering on every rank (collective).  Each row lives on exactly one
        shard: every rank fills in the rows it owns and ONE sum all-reduce of the zero-filled blocks completes them
        (save / backup / compaction paths only -- never on the search path)."""
        out = np.zeros((int(n), self.d), dtype=np.float32)
        for l0, g0, m in self._overlaps(row0, n):
            out[g0 - row0:g0 - row0 + m] = self.local.reconstruct_n(l0, m)
        return self._sum_over_ranks(out)

    def reconstruct_batch(self, ids) -> np.ndarray:
        """``IndexFlat.reconstruct_batch`` in GLOBAL numbering on every rank (collective): the owner of each row
        contributes it (gathered on its device), the others zeros, and ONE sum all-reduce completes the block."""
        from .flat_index import ids_as_int64

        a = ids_as_int64(ids, "reconstruct_batch")
        self._check_ids("reconstruct_batch", a)
        out = np.zeros((a.shape[0], self.d), dtype=np.float32)
        loc = self._local_ids(a)
        own = np.flatnonzero(loc >= 0)
        if own.size:
            # (one segment: the local index adds id_base itself, so it is asked by global id)
            ask = a[own] if len(self.segments) == 1 else loc[own]
            out[own] = self.local.reconstruct_batch(ask)
        return self._sum_over_ranks(out)

    # -- k-means -----------------------------------------------------------------------------------------------------
    def kmeans(self, nc: int, niter: int = 20, seed: int = 0, init=None, spherical: Optional[bool] = None, allow=None,
               max_points_per_centroid: int = 0):
        """``IndexFlat.kmeans`` over the shards (collective: every rank passes the same arguments; ``allow`` is a mask
        over the GLOBAL rows).  The loop is ``flat_index.run_kmeans``; a step is the local ``kmeans_step`` under the
        GLOBAL shift (row counts summed, largest norms reduced with max) followed by ONE sum all-reduce of the int64
        sums, counts and objective (the objective formed from the step's distances at the global ``t``) -- exact integers, so centroids, sizes and objective are bit-identical to one
        index over the same rows.  ``assign`` / ``dist`` of the result are those of THIS shard's rows, in local order."""
        from .flat_index import KmeansStep, fixed_point_objective, kmeans_shift, kmeans_train_mask, run_kmeans

        n = self.ntotal_global
        g = np.ones(n, dtype=bool) if allow is None else np.asarray(allow, dtype=bool)
        if g.shape[0] != n:
            raise ValueError(f"mask has {g.shape[0]} entries, the sharded index {n} rows")
        if self._dead is not None and self._dead.any():
            g = g.copy()
            g[: self._dead.shape[0]] &= ~self._dead
        rows = np.flatnonzero(g).astype(np.int64)
        local_max = float(self.local.bounds()["max_norm2"]) if self.local.ntotal else 0.0
        max_norm2 = local_max if self.world == 1 else float(self._all_gather_host(np.array([local_max], dtype=np.float64)).max())
        s, _, t = kmeans_shift(max_norm2, n)
        if s < 0:
            raise ValueError(f"kmeans: rows too long for the fixed-point sums (shift {s})")
        sph = self.metric == 0 if spherical is None else bool(spherical)
        train = kmeans_train_mask(rows, n, nc, int(max_points_per_centroid), seed)

        def step(cent, mask, want):
            # (the library's objective is scaled by the shard's OWN largest norm, which differs between shards: the
            # objective is formed here, from the step's distances, at the global t)
            st = self.local.kmeans_step(cent, allow=self.local_rows_of(g if mask is None else mask), fx_shift=s,
                                        want_assign=True, want_dist=True)
            obj = fixed_point_objective(st.dist, st.assign, t)
            flat = np.concatenate([st.sums.reshape(-1), st.counts, np.array([obj], dtype=np.int64)])
            flat = self._sum_over_ranks(np.ascontiguousarray(flat, dtype=np.int64))
            m = st.sums.size
            return KmeansStep(flat[:m].reshape(st.sums.shape), flat[m:m + st.counts.size], int(flat[-1]), s, t,
                              st.assign if want else None, st.dist if want else None)

        return run_kmeans(step, self.reconstruct_batch, nc, niter=niter, seed=seed, init=init, spherical=sph,
                          init_rows=rows, train_allow=train, allow=None)

    # -- PCA ---------------------------------------------------------------------------------------------------------
    def gram(self, allow=None, fx_shift: Optional[int] = None):
        """``IndexFlat.gram`` over the shards (collective; ``allow`` is a mask over the GLOBAL rows, tombstones are left
        out): the local Gram matrix under the GLOBAL shift (row counts summed, largest norms reduced with max) and ONE
        sum all-reduce of matrix, column sums and count -- exact integers, bit-identical to one index over the rows.
        One index accepts rows longer than 2^20 (its own shift is then negative); the shards cannot, because
        ``css_index_gram`` reads a negative ``fx_shift`` as "choose": a negative global shift raises ``ValueError``."""
        from .flat_index import GramResult, pca_shift

        n = self.ntotal_global
        local_max = float(self.local.bounds()["max_norm2"]) if self.local.ntotal else 0.0
        max_norm2 = local_max if self.world == 1 else float(self._all_gather_host(np.array([local_max], dtype=np.float64)).max())
        p = pca_shift(max_norm2, n)[0] if fx_shift is None else int(fx_shift)
        if p < 0:
            raise ValueError(f"gram: rows too long for the fixed-point sums (shift {p})")
        g = self.local.gram(allow=self._local_allow(allow), fx_shift=p)
        flat = np.concatenate([g.gram.reshape(-1), g.colsum, np.array([g.count], dtype=np.int64)])
        flat = self._sum_over_ranks(np.ascontiguousarray(flat, dtype=np.int64))
        m = g.gram.size
        return GramResult(flat[:m].reshape(g.gram.shape), flat[m:m + g.colsum.size], int(flat[-1]), p)

    def pca(self, n_components: int, allow=None, whiten: bool = False):
        """``IndexFlat.pca`` over the shards: ``gram`` and ``flat_index.pca_from_gram``, the same bytes on every rank."""
        from .flat_index import pca_from_gram

        g = self.gram(allow=allow)
        return pca_from_gram(g.gram, g.colsum, g.count, g.shift, n_components, whiten=whiten)

    def transform(self, A, b=None, row0: int = 0, n: Optional[int] = None) -> np.ndarray:
        """``IndexFlat.transform`` of the GLOBAL rows ``[row0, row0 + n)`` on every rank (collective), following
        ``reconstruct_n``: every shard transforms the rows it owns and ONE sum all-reduce of the zero-filled blocks
        completes them (exact: one non-zero contribution per row)."""
        from .flat_index import transform_args

        A, b = transform_args(A, b, self.d)
        row0 = int(row0)
        n = self.ntotal_global - row0 if n is None else int(n)
        if n < 0:
            raise ValueError(f"transform: n={n} is negative")
        self._check_rows("transform", row0, n)
        out = np.zeros((n, A.shape[0]), dtype=np.float32)
        for l0, g0, m in self._overlaps(row0, n):
            out[g0 - row0:g0 - row0 + m] = self.local.transform(A, b, l0, m)
        return self._sum_over_ranks(out)

    def add_file_rows(self, path: str, offset: int, n: int, normalize: bool = False, chunk_rows: int = 1 << 18) -> None:
        """``add_global`` of ``n`` fp32 rows stored row-major at byte ``offset`` of ``path`` (the payload of an index
        file): every rank reads only its own block (collective call, no communication)."""
        bounds = [shard_bounds(n, self.world, r) for r in range(self.world)]
        lo, hi = bounds[self.rank]
        if hi > lo:
            if self.shard_sizes[self.rank] == 0:
                self.local.reserve(hi - lo)
            with open(path, "rb") as f:
                for r0 in range(lo, hi, chunk_rows):
                    m = min(chunk_rows, hi - r0)
                    f.seek(offset + r0 * self.d * 4)
                    buf = f.read(m * self.d * 4)
                    if len(buf) != m * self.d * 4:
                        raise RuntimeError("truncated index file (in rows)")
                    self.local.add(np.frombuffer(buf, dtype=np.float32).reshape(m, self.d), normalize=normalize)
        self._append_segment(hi - lo, self.ntotal_global + lo)
        self._account([b[1] - b[0] for b in bounds], n)


class ShardedIndexFacade:
    """The members of ``flat_index.IndexFlat`` that ``HybridStorage`` touches, over a ``ShardedFlatIndex``: the
    reference's ``Storage.search()`` behind 1..8 GPUs (``StorageConfig.sharded``).  SPMD: every rank of the process
    group runs the same ``HybridStorage`` calls with the same arguments (adds, searches, deletes, saves); an ``add`` of
    a file's chunks goes whole to the least-full shard (``add_routed``), a search is the local masked search + ONE
    all-gather + merge, and ids are those of one ``IndexFlat`` that received the same calls."""

    def __init__(self, d: int, metric: int = 0, device: int = 0, group=None, index_factory=None, merge=None):
        self.sh = ShardedFlatIndex(d, metric, group=group, device_index=device, index_factory=index_factory, merge=merge)
        self.d, self.metric_type, self.device, self.is_trained = int(d), int(metric), int(device), True

    ntotal = property(lambda self: self.sh.ntotal_global)

    def reserve(self, n: int) -> None:   # (shards grow on their own; a global reserve would over-allocate every shard)
        pass

    def add(self, x, normalize: bool = False) -> None:
        a = np.ascontiguousarray(x, dtype=np.float32).reshape(-1, self.d)
        if a.shape[0]:
            self.sh.add_routed(a, normalize=normalize)

    def search(self, q, k: int, normalize: bool = False, allow=None):
        return self.sh.search(np.asarray(q, dtype=np.float32), int(k), normalize=normalize, allow=allow)

    def range_search(self, q, thresh: float, normalize: bool = False, allow=None):
        return self.sh.range_search(np.asarray(q, dtype=np.float32), float(thresh), normalize=normalize, allow=allow)

    def search_by_ids(self, ids, k: int, exclude_self: bool = True, allow=None):
        return self.sh.search_by_ids(ids, int(k), exclude_self=exclude_self, allow=allow)

    def set_groups(self, labels, row0: int = 0) -> None:
        self.sh.set_groups(labels, row0=row0)

    def search_grouped(self, q, k: int, normalize: bool = False, allow=None):
        return self.sh.search_grouped(np.asarray(q, dtype=np.float32), int(k), normalize=normalize, allow=allow)

    def set_priors(self, priors, row0: int = 0) -> None:
        self.sh.set_priors(priors, row0=row0)

    def search_prior(self, q, k: int, weight: float, normalize: bool = False, allow=None):
        return self.sh.search_prior(np.asarray(q, dtype=np.float32), int(k), float(weight), normalize=normalize, allow=allow)

    def search_examples(self, pos=None, neg=None, pos_ids=(), neg_ids=(), k: int = 10, gamma: float = 0.5,
                        normalize: bool = False, exclude_ids: bool = True, allow=None):
        return self.sh.search_examples(pos, neg, pos_ids, neg_ids, k=int(k), gamma=float(gamma), normalize=normalize,
                                       exclude_ids=exclude_ids, allow=allow)

    def set_terms(self, lists, row0: Optional[int] = None) -> None:
        self.sh.set_terms(lists, row0=row0)

    def term_stats(self, terms):
        return self.sh.term_stats(terms)

    def subset_terms(self, allow=None):
        return self.sh.subset_terms(allow=allow)

    def significant_terms(self, allow=None, m: int = 20, min_count: int = 2, background=None):
        return self.sh.significant_terms(allow=allow, m=m, min_count=min_count, background=background)

    def facets(self, q, thresh: float, buckets=None, nbuckets=None, normalize: bool = False, allow=None, by_attribute=None):
        return self.sh.facets(np.asarray(q, dtype=np.float32), float(thresh), buckets=buckets, nbuckets=nbuckets,
                              normalize=normalize, allow=allow, by_attribute=by_attribute)

    def set_attribute(self, slot: int, values, row0: int = 0) -> None:
        self.sh.set_attribute(slot, values, row0=row0)

    def get_attribute(self, slot: int) -> np.ndarray:
        return self.sh.get_attribute(slot)

    def attribute_type(self, slot: int) -> int:
        return self.sh.attribute_type(slot)

    def drop_attribute(self, slot: int) -> None:
        self.sh.drop_attribute(slot)

    def where(self, clauses, allow=None, return_count: bool = False):
        return self.sh.where(clauses, allow=allow, return_count=return_count)

    def search_hybrid(self, q, terms, weights, k: int, alpha: float, k1: float = 1.2, b: float = 0.75,
                      avgdl: Optional[float] = None, normalize: bool = False, allow=None):
        return self.sh.search_hybrid(np.asarray(q, dtype=np.float32), terms, weights, int(k), float(alpha), k1=k1, b=b,
                                     avgdl=avgdl, normalize=normalize, allow=allow)

    def set_sparse(self, vectors, row0: Optional[int] = None) -> None:
        self.sh.set_sparse(vectors, row0=row0)

    @property
    def sparse_rows(self) -> int:
        return self.sh.sparse_rows

    def search_sparse(self, terms, weights, k: int, allow=None):
        return self.sh.search_sparse(terms, weights, int(k), allow=allow)

    def search_hybrid_sparse(self, q, terms, weights, k: int, alpha: float, normalize: bool = False, allow=None):
        return self.sh.search_hybrid_sparse(np.asarray(q, dtype=np.float32), terms, weights, int(k), float(alpha),
                                            normalize=normalize, allow=allow)

    def set_tokens(self, mats, keep=None, row0: Optional[int] = None) -> None:
        self.sh.set_tokens(mats, keep=keep, row0=row0)

    def get_tokens(self, row0: int = 0, n: Optional[int] = None):
        return self.sh.get_tokens(row0, n)

    @property
    def token_rows(self) -> int:
        return self.sh.token_rows

    @property
    def token_dim(self) -> int:
        return self.sh.token_dim

    def drop_tokens(self) -> None:
        self.sh.drop_tokens()

    def set_token_codec(self, codec) -> None:
        self.sh.set_token_codec(codec)

    @property
    def token_codec_bits(self) -> int:
        return self.sh.token_codec_bits

    def get_token_codec(self):
        return self.sh.get_token_codec()

    def get_token_codes(self, row0: int = 0, n: Optional[int] = None):
        return self.sh.get_token_codes(row0, n)

    def set_token_codes(self, offsets, codes, res, row0: Optional[int] = None) -> None:
        self.sh.set_token_codes(offsets, codes, res, row0=row0)

    def search_maxsim(self, q_mat, k: int, allow=None):
        return self.sh.search_maxsim(q_mat, int(k), allow=allow)

    def search_maxsim_batch(self, q_mats, k: int, allow=None):
        return self.sh.search_maxsim_batch(q_mats, int(k), allow=allow)

    def maxsim_ids(self, q_mat, ids) -> np.ndarray:
        return self.sh.maxsim_ids(q_mat, ids)

    def maxsim_ids_batch(self, q_mats, ids) -> np.ndarray:
        return self.sh.maxsim_ids_batch(q_mats, ids)

    def search_rerank_maxsim(self, q, q_mats, k: int, fetch: int, normalize: bool = False, floor=None, allow=None):
        return self.sh.search_rerank_maxsim(q, q_mats, int(k), int(fetch), normalize=normalize, floor=floor, allow=allow)

    def maxsim_candidates(self, q_mat, ncand: int, allow=None):
        return self.sh.maxsim_candidates(q_mat, int(ncand), allow=allow)

    def search_maxsim_pruned(self, q_mat, k: int, ncand: int, allow=None):
        return self.sh.search_maxsim_pruned(q_mat, int(k), int(ncand), allow=allow)

    def search_diverse(self, q, k: int, lam: float = 0.5, fetch: int = 0, normalize: bool = False, allow=None):
        return self.sh.search_diverse(np.asarray(q, dtype=np.float32), int(k), lam=lam, fetch=fetch, normalize=normalize,
                                      allow=allow)

    def reconstruct_n(self, row0: int = 0, n: Optional[int] = None) -> np.ndarray:
        return self.sh.reconstruct_n(int(row0), self.ntotal - int(row0) if n is None else int(n))

    def reconstruct(self, i: int) -> np.ndarray:
        return self.reconstruct_n(int(i), 1)[0]

    def reconstruct_batch(self, ids) -> np.ndarray:
        return self.sh.reconstruct_batch(ids)

    def kmeans(self, nc: int, niter: int = 20, seed: int = 0, init=None, spherical: Optional[bool] = None, allow=None,
               max_points_per_centroid: int = 0):
        """``ShardedFlatIndex.kmeans`` with ``assign`` / ``dist`` in GLOBAL numbering on every rank, as one ``IndexFlat``
        would return them (every shard fills in its rows; one sum all-reduce)."""
        res = self.sh.kmeans(nc, niter=niter, seed=seed, init=init, spherical=spherical, allow=allow,
                             max_points_per_centroid=max_points_per_centroid)
        a = np.zeros(self.ntotal, dtype=np.int64)
        d = np.zeros(self.ntotal, dtype=np.float32)
        for l0, g0, n in self.sh._overlaps(0, self.ntotal):
            a[g0:g0 + n] = res.assign[l0:l0 + n].astype(np.int64) + 1   # (0 = not this shard's row)
            d[g0:g0 + n] = res.dist[l0:l0 + n]
        a, d = self.sh._sum_over_ranks(a), self.sh._sum_over_ranks(d)
        return res._replace(assign=(a - 1).astype(np.int32), dist=d)

    def gram(self, allow=None, fx_shift: Optional[int] = None):
        return self.sh.gram(allow=allow, fx_shift=fx_shift)

    def pca(self, n_components: int, allow=None, whiten: bool = False):
        return self.sh.pca(int(n_components), allow=allow, whiten=whiten)

    def transform(self, A, b=None, row0: int = 0, n: Optional[int] = None) -> np.ndarray:
        return self.sh.transform(A, b, row0=row0, n=n)

    def mark_deleted(self, ids) -> None:
        self.sh.mark_deleted(ids)

    def set_search_mode(self, mode: str) -> None:
        self.sh.local.set_search_mode(mode)

    def close(self) -> None:
        self.sh.local.close()


def read_index_sharded(path: str, device: int = 0, group=None, index_factory=None, merge=None) -> ShardedIndexFacade:
    """``flat_index.read_index`` for a shard group: the header is validated by the same code, then every rank reads
    its own contiguous block of the rows (global ids = file order, as ``faiss.read_index`` numbers them)."""
    from . import flat_index as fi

    d, n, metric, offset = fi.read_index_header(path)
    ix = ShardedIndexFacade(d, metric, device=device, group=group, index_factory=index_factory, merge=merge)
    if n:
        ix.sh.add_file_rows(path, offset, n)
    return ix
