"""The product-quantized row store (Jegou et al., 2011; the compression MUVERA applies to its encodings): a dense row of
``d`` components kept as ``M = d / 8`` bytes, byte ``m`` the number of one of the 256 bf16 centroids of sub-quantizer
``m``, and scanned exhaustively on the codes.  ``include/css_hip.h`` defines encoding and score in bits.

``ProductQuantizer`` holds the codebooks and restates the definition in numpy (``encode_numpy`` in float32 gives the
device's bytes, ``scores_numpy`` is float64); ``IndexPQ`` is the store on the GPU (``css_pq_*``, kernels in
``csrc/css_pq.h``); ``train_product_quantizer`` makes codebooks from a sample with the index's k-means."""
from __future__ import annotations

import ctypes
from typing import Optional, Tuple

import numpy as np

from . import _native as nat
from .flat_index import IndexFlatL2, bf16_to_f32, f32_to_bf16_rne, pack_allow_bits

MAX_DIM = 8192        # css_pq_create's limit on d
MAX_K = 128           # css_pq_search's limit on k
MAX_QUERIES = 65536   # include/css_hip.h CSS_PQ_MAX_QUERIES
SUB = 8               # components of a sub-vector
NCENT = 256           # centroids of a sub-quantizer


def pq_dim(d: int) -> int:
    """The checked row width; returns ``M = d / 8``.  What the library would refuse raises here."""
    d = int(d)
    if not (32 <= d <= MAX_DIM and d % 32 == 0):
        raise ValueError(f"pq: d={d} must be a multiple of 32 in [32, {MAX_DIM}]")
    return d // SUB


class ProductQuantizer:
    """The codebooks: float32 ``[M, 256, 8]`` from the caller, kept as the bf16 values (round to nearest even) that the
    library keeps.  ``codebooks`` is that float32 array; passing it again changes nothing."""

    def __init__(self, d: int, codebooks):
        self.d, self.M = int(d), pq_dim(d)
        c = np.ascontiguousarray(codebooks, dtype=np.float32)
        if c.shape != (self.M, NCENT, SUB):
            raise ValueError(f"pq: codebooks has shape {c.shape}, not {(self.M, NCENT, SUB)}")
        if not np.isfinite(c).all():
            raise ValueError("pq: codebooks holds a NaN or infinite component")
        bits = f32_to_bf16_rne(c)
        if ((bits & 0x7F80) == 0x7F80).any():
            raise ValueError("pq: a component of codebooks is infinite once rounded to bf16")
        self.codebooks = bf16_to_f32(bits).reshape(c.shape)

    def _rows(self, x, what: str) -> np.ndarray:
        a = np.ascontiguousarray(x, dtype=np.float32)
        if a.ndim != 2 or a.shape[1] != self.d:
            raise ValueError(f"{what}: expected shape [n, {self.d}], got {a.shape}")
        if not np.isfinite(a).all():
            raise ValueError(f"{what}: a component is NaN or infinite")
        return a

    def _codes(self, codes, what: str) -> np.ndarray:
        c = np.ascontiguousarray(codes)
        if c.dtype != np.uint8 or c.ndim != 2 or c.shape[1] != self.M:
            raise ValueError(f"{what}: codes must be uint8 [n, {self.M}], got {c.dtype} {c.shape}")
        return c

    def encode_numpy(self, x, dtype=np.float32) -> np.ndarray:
        """``code[m] = argmin_c sum_j (x[8 m + j] - c[j])^2``, uint8 ``[n, M]``: in ``dtype`` arithmetic, one rounding
        per operation, ``j`` ascending from 0, ties to the lower ``c`` (``argmin`` takes the first).  float32 is the
        device's chain; float64 is the reference it is compared with."""
        a = self._rows(x, "encode_numpy").reshape(-1, self.M, SUB).astype(dtype)
        out = np.empty((a.shape[0], self.M), dtype=np.uint8)
        for m in range(self.M):
            cb = self.codebooks[m].astype(dtype)                      # [256, 8]
            acc = np.zeros((a.shape[0], NCENT), dtype=dtype)
            for j in range(SUB):
                t = a[:, m, j, None] - cb[None, :, j]
                acc = acc + t * t
            out[:, m] = acc.argmin(axis=1)
        return out

    def decode_numpy(self, codes) -> np.ndarray:
        """The rows the codes stand for: float32 ``[n, d]`` of (bf16-exact) centroid components."""
        c = self._codes(codes, "decode_numpy")
        return self.codebooks[np.arange(self.M)[None, :], c].reshape(c.shape[0], self.d)

    def scores_numpy(self, q, codes) -> np.ndarray:
        """``s(q, r) = sum_i bf16_rne(q_i) * decode(r)_i`` in float64: ``[nq, n]``."""
        qh = bf16_to_f32(f32_to_bf16_rne(self._rows(q, "scores_numpy"))).reshape(-1, self.d)
        return qh.astype(np.float64) @ self.decode_numpy(codes).astype(np.float64).T


def search_numpy(scores, k: int, allow=None) -> Tuple[np.ndarray, np.ndarray]:
    """The ranking of ``IndexPQ.search`` from a score matrix ``[nq, n]``: best first, ties to the lower id, the rows
    outside ``allow`` left out, padded with ``-FLT_MAX`` / ``-1``."""
    s = np.asarray(scores)
    nq, n = s.shape
    D = np.full((nq, k), -np.finfo(np.float32).max, dtype=np.float32)
    I = np.full((nq, k), -1, dtype=np.int64)
    ids = np.arange(n) if allow is None else np.flatnonzero(np.asarray(allow))
    for b in range(nq):
        order = ids[np.lexsort((ids, -s[b, ids]))][:k]
        D[b, :order.size], I[b, :order.size] = s[b, order], order
    return D, I


class IndexPQ:
    """The store on the GPU.  ``codebooks``: float32 ``[d / 8, 256, 8]`` or a ``ProductQuantizer``.  Rows are numbered
    in the order they were added; nothing but their codes is kept."""

    def __init__(self, d: int, codebooks, device: int = 0):
        self._h: Optional[ctypes.c_void_p] = None
        self.pq = codebooks if isinstance(codebooks, ProductQuantizer) else ProductQuantizer(d, codebooks)
        if self.pq.d != int(d):
            raise ValueError(f"pq: the quantizer has d={self.pq.d}, the index d={int(d)}")
        self.d, self.M, self.device = self.pq.d, self.pq.M, int(device)
        h = ctypes.c_void_p()
        nat.check(nat.lib().css_pq_create(self.d, self.pq.codebooks.ctypes.data, self.device, ctypes.byref(h)))
        self._h = h

    def close(self) -> None:
        if getattr(self, "_h", None) is not None:
            nat.lib().css_pq_free(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):  # pragma: no cover - interpreter shutdown order
        try:
            self.close()
        except Exception:
            pass

    def _handle(self):
        if self._h is None:
            raise RuntimeError("the store has been freed")
        return self._h

    @property
    def ntotal(self) -> int:
        n = ctypes.c_int64(0)
        nat.check(nat.lib().css_pq_ntotal(self._handle(), ctypes.byref(n)))
        return int(n.value)

    @property
    def last_passes(self) -> int:
        """The scans of the codes the last search made: ``ceil(nq / 16)``."""
        p = ctypes.c_int(0)
        nat.check(nat.lib().css_pq_last_passes(self._handle(), ctypes.byref(p)))
        return int(p.value)

    def add(self, x) -> None:
        """Encode float32 rows ``[n, d]`` on the device and append their codes."""
        a = self.pq._rows(x, "add")
        if a.shape[0]:
            nat.check(nat.lib().css_pq_add(self._handle(), a.ctypes.data, a.shape[0]))

    def add_dev(self, x) -> None:
        """``add`` from a contiguous float32 torch tensor ``[n, d]`` on the store's device, enqueued on torch's current
        stream (``css_pq_add_dev``): the codes of the host form."""
        import torch

        if x.dtype != torch.float32 or x.dim() != 2 or x.shape[1] != self.d or not x.is_contiguous():
            raise ValueError(f"add_dev: expected a contiguous float32 tensor [n, {self.d}]")
        if x.device != torch.device("cuda", self.device):
            raise ValueError(f"add_dev: the tensor is on {x.device}, the store on device {self.device}")
        if x.shape[0]:
            st = torch.cuda.current_stream(x.device).cuda_stream
            nat.check(nat.lib().css_pq_add_dev(self._handle(), x.data_ptr(), x.shape[0], ctypes.c_void_p(st)))

    def add_codes(self, codes) -> None:
        """Append rows that are codes already: uint8 ``[n, M]``, the form ``get_codes`` returns."""
        c = self.pq._codes(codes, "add_codes")
        if c.shape[0]:
            nat.check(nat.lib().css_pq_add_codes(self._handle(), c.ctypes.data, c.shape[0]))

    def _range(self, row0: int, n: Optional[int]) -> Tuple[int, int]:
        row0 = int(row0)
        return row0, self.ntotal - row0 if n is None else int(n)

    def get_codes(self, row0: int = 0, n: Optional[int] = None) -> np.ndarray:
        row0, n = self._range(row0, n)
        out = np.empty((max(n, 0), self.M), dtype=np.uint8)
        nat.check(nat.lib().css_pq_get_codes(self._handle(), row0, n, out.ctypes.data))
        return out

    def reconstruct_n(self, row0: int = 0, n: Optional[int] = None) -> np.ndarray:
        """Rows ``[row0, row0 + n)`` decoded on the device: float32 ``[n, d]``, ``decode_numpy`` of their codes."""
        row0, n = self._range(row0, n)
        out = np.empty((max(n, 0), self.d), dtype=np.float32)
        nat.check(nat.lib().css_pq_reconstruct(self._handle(), row0, n, out.ctypes.data))
        return out

    def _search_args(self, nq: int, k: int) -> int:
        k = int(k)
        if not 1 <= k <= MAX_K:
            raise ValueError(f"search: k={k} outside [1, {MAX_K}]")
        if nq > MAX_QUERIES:
            raise ValueError(f"search: nq={nq} exceeds {MAX_QUERIES}")
        return k

    def search(self, q, k: int, allow=None) -> Tuple[np.ndarray, np.ndarray]:
        """``(D float32, I int64)``, each ``[nq, k]``: the ``k`` best rows by the inner product of the bf16-rounded
        query with the decoded row, best first, ties to the lower id; ``allow`` is a boolean mask over the rows.
        Padding: ``-FLT_MAX`` / ``-1``.  ``1 <= k <= 128``."""
        a = self.pq._rows(q, "search")
        k = self._search_args(a.shape[0], k)
        if ((f32_to_bf16_rne(a) & 0x7F80) == 0x7F80).any():
            raise ValueError("search: a component is infinite once rounded to bf16")
        D, I = np.empty((a.shape[0], k), dtype=np.float32), np.empty((a.shape[0], k), dtype=np.int64)
        bits = None if allow is None else pack_allow_bits(allow, self.ntotal)
        if a.shape[0]:
            nat.check(nat.lib().css_pq_search(self._handle(), a.ctypes.data, a.shape[0], k,
                                              None if bits is None else bits.ctypes.data, D.ctypes.data, I.ctypes.data))
        return D, I

    def search_dev(self, q, k: int, allow=None):
        """``search`` with a float32 torch tensor ``[nq, d]`` on the store's device, enqueued on torch's current stream
        (``css_pq_search_dev``): ``(D, I)`` as torch tensors there, the bytes of the host form.  The contents of ``q``
        are not checked."""
        import torch

        if q.dtype != torch.float32 or q.dim() != 2 or q.shape[1] != self.d or not q.is_contiguous() or q.shape[0] < 1:
            raise ValueError(f"search_dev: expected a contiguous float32 tensor [nq >= 1, {self.d}]")
        dev = torch.device("cuda", self.device)
        if q.device != dev:
            raise ValueError(f"search_dev: the tensor is on {q.device}, the store on device {self.device}")
        k = self._search_args(q.shape[0], k)
        D = torch.empty((q.shape[0], k), dtype=torch.float32, device=dev)
        I = torch.empty((q.shape[0], k), dtype=torch.int64, device=dev)
        bits = None
        if allow is not None:
            bits = torch.from_numpy(pack_allow_bits(allow, self.ntotal).view(np.int32)).to(dev)
        st = torch.cuda.current_stream(dev).cuda_stream
        nat.check(nat.lib().css_pq_search_dev(self._handle(), q.data_ptr(), q.shape[0], k,
                                              None if bits is None else bits.data_ptr(), D.data_ptr(), I.data_ptr(),
                                              ctypes.c_void_p(st)))
        return D, I


def train_product_quantizer(x, niter: int = 20, seed: int = 0, device: int = 0) -> ProductQuantizer:
    """Codebooks from a sample ``x [n >= 256, d]``: per sub-space the GPU k-means of the flat index
    (``IndexFlatL2(8).kmeans(256)``) over the sample's sub-vectors.  A convenience, one small clustering after the
    other; the same call gives the same codebooks."""
    a = np.ascontiguousarray(x, dtype=np.float32)
    if a.ndim != 2:
        raise ValueError(f"train_product_quantizer: expected a 2-D sample, got shape {a.shape}")
    M = pq_dim(a.shape[1])
    if a.shape[0] < NCENT:
        raise ValueError(f"train_product_quantizer: {a.shape[0]} sample rows for {NCENT} centroids")
    if not np.isfinite(a).all():
        raise ValueError("train_product_quantizer: a component is NaN or infinite")
    cb = np.empty((M, NCENT, SUB), dtype=np.float32)
    for m in range(M):
        ix = IndexFlatL2(SUB, device)
        try:
            ix.add(np.ascontiguousarray(a[:, SUB * m:SUB * (m + 1)]))
            cb[m] = ix.kmeans(NCENT, niter=niter, seed=seed + m, spherical=False).centroids
        finally:
            ix.close()
    return ProductQuantizer(a.shape[1], cb)
