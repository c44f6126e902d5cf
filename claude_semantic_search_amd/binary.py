"""The binary row store (``faiss.IndexBinaryFlat``; the ``ubinary`` precision of sentence-transformers): a dense row of
``d`` components kept as ``d`` sign bits, ``d / 8`` bytes, and scanned exhaustively by Hamming distance.  Training-free,
and integers throughout: ``include/css_hip.h`` defines code, distance and ranking in bits.

``binarize_numpy``, ``hamming_numpy`` and ``search_numpy`` restate the definition in numpy; ``IndexBinaryFlat`` is the
store on the GPU (``css_bin_*``, kernels in ``csrc/css_binary.h``)."""
from __future__ import annotations

import ctypes
from typing import Optional, Tuple

import numpy as np

from . import _native as nat
from .flat_index import pack_allow_bits

MAX_DIM = 8192        # css_bin_create's limit on d
MAX_K = 128           # the searches' limit on k
MAX_QUERIES = 65536   # include/css_hip.h CSS_BIN_MAX_QUERIES
MAX_WAVES = 16384     # include/css_hip.h CSS_BIN_MAX_WAVES
PAD_DISTANCE = np.iinfo(np.int32).max


def binary_dim(d: int) -> int:
    """The checked row width; returns the bytes of a code, ``d / 8``.  What the library would refuse raises here."""
    d = int(d)
    if not (32 <= d <= MAX_DIM and d % 32 == 0):
        raise ValueError(f"binary: d={d} must be a multiple of 32 in [32, {MAX_DIM}]")
    return d // 8


def binarize_numpy(x) -> np.ndarray:
    """The code of float rows ``[n, d]``: bit ``i`` is ``x[i] > 0``, packed big-endian within a byte -- uint8 ``[n, d / 8]``."""
    return np.packbits(np.asarray(x) > 0, axis=-1)


def hamming_numpy(qc, rc) -> np.ndarray:
    """``popcount(code_q xor code_r)`` of codes ``[nq, d / 8]`` and ``[n, d / 8]``: int64 ``[nq, n]``."""
    qc, rc = np.asarray(qc, dtype=np.uint8), np.asarray(rc, dtype=np.uint8)
    ones = np.unpackbits(np.arange(256, dtype=np.uint8)[:, None], axis=1).sum(1)   # the set bits of every byte value
    return np.array([ones[q[None, :] ^ rc].sum(1) for q in qc], dtype=np.int64).reshape(qc.shape[0], rc.shape[0])


def search_numpy(dist, k: int, allow=None) -> Tuple[np.ndarray, np.ndarray]:
    """The ranking of ``IndexBinaryFlat.search`` from distances ``[nq, n]``: smallest first, ties to the lower id, the
    rows outside ``allow`` left out, padded with ``INT32_MAX`` / ``-1``."""
    h = np.asarray(dist)
    nq, n = h.shape
    D = np.full((nq, k), PAD_DISTANCE, dtype=np.int32)
    I = np.full((nq, k), -1, dtype=np.int64)
    ids = np.arange(n) if allow is None else np.flatnonzero(np.asarray(allow))
    for b in range(nq):
        order = ids[np.lexsort((ids, h[b, ids]))][:k]
        D[b, :order.size], I[b, :order.size] = h[b, order], order
    return D, I


PAD_SCORE = np.iinfo(np.int32).min


def quantize_queries_numpy(q) -> Tuple[np.ndarray, np.ndarray]:
    """The int8 form of float queries ``[nq, d]`` as ``search_asym_float`` makes it, in float32 throughout:
    ``a = max |q_i|``; all zeros if ``a`` is below the smallest normal float, else ``rint((q_i / a) * 127)``.  Returns
    ``(q8 int8 [nq, d], a float32 [nq])``; ``a * score / 127`` estimates the float query's product with the signs."""
    q = np.ascontiguousarray(q, dtype=np.float32)
    a = np.abs(q).max(axis=1) if q.shape[1] else np.zeros(q.shape[0], np.float32)
    live = a.view(np.int32) >= 0x00800000
    q8 = np.zeros(q.shape, dtype=np.int8)
    with np.errstate(under="ignore"):
        q8[live] = np.rint((q[live] / a[live, None]) * np.float32(127)).astype(np.int8)
    return q8, a


def asym_scores_numpy(q8, codes) -> np.ndarray:
    """``sum_i q8_i (2 b_i - 1)`` of int8 queries ``[nq, d]`` against codes ``[n, d / 8]``: int64 ``[nq, n]``."""
    signs = 2 * np.unpackbits(np.asarray(codes, dtype=np.uint8), axis=-1).astype(np.int32) - 1
    return (np.asarray(q8, dtype=np.int8).astype(np.int32) @ signs.T).astype(np.int64)   # (|s| <= 2^20: exact in int32)


def search_asym_numpy(scores, k: int, allow=None) -> Tuple[np.ndarray, np.ndarray]:
    """The ranking of ``IndexBinaryFlat.search_asym`` from scores ``[nq, n]``: largest first, ties to the lower id, the
    rows outside ``allow`` left out, padded with ``INT32_MIN`` / ``-1``."""
    s = np.asarray(scores)
    nq, n = s.shape
    D = np.full((nq, k), PAD_SCORE, dtype=np.int32)
    I = np.full((nq, k), -1, dtype=np.int64)
    ids = np.arange(n) if allow is None else np.flatnonzero(np.asarray(allow))
    for b in range(nq):
        order = ids[np.lexsort((ids, -s[b, ids]))][:k]
        D[b, :order.size], I[b, :order.size] = s[b, order], order
    return D, I


class IndexBinaryFlat:
    """The store on the GPU, in the faiss shape: ``add`` / ``search`` take codes (uint8 ``[n, d / 8]``),
    ``add_float`` / ``search_float`` take float32 rows and binarize them on the device.  Rows are numbered in the order
    they were added."""

    def __init__(self, d: int, device: int = 0):
        self._h: Optional[ctypes.c_void_p] = None
        self.code_size = binary_dim(d)
        self.d, self.device = int(d), int(device)
        h = ctypes.c_void_p()
        nat.check(nat.lib().css_bin_create(self.d, self.device, ctypes.byref(h)))
        self._h = h

    def close(self) -> None:
        if getattr(self, "_h", None) is not None:
            nat.lib().css_bin_free(self._h)
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
        nat.check(nat.lib().css_bin_ntotal(self._handle(), ctypes.byref(n)))
        return int(n.value)

    @property
    def last_passes(self) -> int:
        """The scans of the codes the last search made: ``ceil(nq / 16)``."""
        p = ctypes.c_int(0)
        nat.check(nat.lib().css_bin_last_passes(self._handle(), ctypes.byref(p)))
        return int(p.value)

    def set_waves(self, waves: int) -> None:
        """The number of scanning waves (row ranges) of the next searches, 0 = automatic.  No answer depends on it."""
        waves = int(waves)
        if not 0 <= waves <= MAX_WAVES:
            raise ValueError(f"set_waves: waves={waves} outside [0, {MAX_WAVES}]")
        nat.check(nat.lib().css_bin_set_waves(self._handle(), waves))

    # ---- argument checks
    def _codes(self, codes, what: str) -> np.ndarray:
        c = np.ascontiguousarray(codes)
        if c.dtype != np.uint8 or c.ndim != 2 or c.shape[1] != self.code_size:
            raise ValueError(f"{what}: codes must be uint8 [n, {self.code_size}], got {c.dtype} {c.shape}")
        return c

    def _rows(self, x, what: str) -> np.ndarray:
        a = np.ascontiguousarray(x, dtype=np.float32)
        if a.ndim != 2 or a.shape[1] != self.d:
            raise ValueError(f"{what}: expected shape [n, {self.d}], got {a.shape}")
        if not np.isfinite(a).all():
            raise ValueError(f"{what}: a component is NaN or infinite")
        return a

    def _search_args(self, nq: int, k: int) -> int:
        k = int(k)
        if not 1 <= k <= MAX_K:
            raise ValueError(f"search: k={k} outside [1, {MAX_K}]")
        if nq > MAX_QUERIES:
            raise ValueError(f"search: nq={nq} exceeds {MAX_QUERIES}")
        return k

    def _tensor(self, t, dtype, width: int, what: str, min_rows: int):
        import torch

        if t.dtype != dtype or t.dim() != 2 or t.shape[1] != width or not t.is_contiguous() or t.shape[0] < min_rows:
            raise ValueError(f"{what}: expected a contiguous {dtype} tensor [n >= {min_rows}, {width}]")
        dev = torch.device("cuda", self.device)
        if t.device != dev:
            raise ValueError(f"{what}: the tensor is on {t.device}, the store on device {self.device}")
        return dev

    # ---- rows
    def add(self, codes) -> None:
        """Append rows that are codes: uint8 ``[n, d / 8]``, ``np.packbits`` order."""
        c = self._codes(codes, "add")
        if c.shape[0]:
            nat.check(nat.lib().css_bin_add_codes(self._handle(), c.ctypes.data, c.shape[0]))

    def add_float(self, x) -> None:
        """Binarize float32 rows ``[n, d]`` on the device (``x > 0``) and append their codes."""
        a = self._rows(x, "add_float")
        if a.shape[0]:
            nat.check(nat.lib().css_bin_add(self._handle(), a.ctypes.data, a.shape[0]))

    def add_dev(self, x) -> None:
        """``add_float`` from a contiguous float32 torch tensor ``[n, d]`` on the store's device, enqueued on torch's
        current stream (``css_bin_add_dev``).  The contents are not checked."""
        import torch

        dev = self._tensor(x, torch.float32, self.d, "add_dev", 0)
        if x.shape[0]:
            st = torch.cuda.current_stream(dev).cuda_stream
            nat.check(nat.lib().css_bin_add_dev(self._handle(), x.data_ptr(), x.shape[0], ctypes.c_void_p(st)))

    def get_codes(self, row0: int = 0, n: Optional[int] = None) -> np.ndarray:
        """The codes of rows ``[row0, row0 + n)``: uint8 ``[n, d / 8]``."""
        row0 = int(row0)
        n = self.ntotal - row0 if n is None else int(n)
        out = np.empty((max(n, 0), self.code_size), dtype=np.uint8)
        nat.check(nat.lib().css_bin_get_codes(self._handle(), row0, n, out.ctypes.data))
        return out

    # ---- searches
    def _search_host(self, fn, a: np.ndarray, k: int, allow) -> Tuple[np.ndarray, np.ndarray]:
        k = self._search_args(a.shape[0], k)
        D, I = np.empty((a.shape[0], k), dtype=np.int32), np.empty((a.shape[0], k), dtype=np.int64)
        bits = None if allow is None else pack_allow_bits(allow, self.ntotal)
        if a.shape[0]:
            nat.check(fn(self._handle(), a.ctypes.data, a.shape[0], k, None if bits is None else bits.ctypes.data,
                         D.ctypes.data, I.ctypes.data))
        return D, I

    def search(self, codes, k: int, allow=None) -> Tuple[np.ndarray, np.ndarray]:
        """``(D int32, I int64)``, each ``[nq, k]``: the ``k`` rows at the smallest Hamming distance from each query
        code, smallest first, ties to the lower id; ``allow`` is a boolean mask over the rows.  Padding:
        ``INT32_MAX`` / ``-1``.  ``1 <= k <= 128``."""
        return self._search_host(nat.lib().css_bin_search_codes, self._codes(codes, "search"), k, allow)

    def search_float(self, q, k: int, allow=None) -> Tuple[np.ndarray, np.ndarray]:
        """``search`` of float32 queries ``[nq, d]``, binarized on the device like the rows of ``add_float``."""
        return self._search_host(nat.lib().css_bin_search, self._rows(q, "search_float"), k, allow)

    def _search_dev(self, fn, q, dev, k: int, allow):
        import torch

        k = self._search_args(q.shape[0], k)
        D = torch.empty((q.shape[0], k), dtype=torch.int32, device=dev)
        I = torch.empty((q.shape[0], k), dtype=torch.int64, device=dev)
        bits = None
        if allow is not None:
            bits = torch.from_numpy(pack_allow_bits(allow, self.ntotal).view(np.int32)).to(dev)
        st = torch.cuda.current_stream(dev).cuda_stream
        nat.check(fn(self._handle(), q.data_ptr(), q.shape[0], k, None if bits is None else bits.data_ptr(), D.data_ptr(),
                     I.data_ptr(), ctypes.c_void_p(st)))
        return D, I

    def search_dev(self, q, k: int, allow=None):
        """``search_float`` with a float32 torch tensor ``[nq, d]`` on the store's device, enqueued on torch's current
        stream (``css_bin_search_dev``): ``(D, I)`` as torch tensors there, the bytes of the host form."""
        import torch

        return self._search_dev(nat.lib().css_bin_search_dev, q, self._tensor(q, torch.float32, self.d, "search_dev", 1), k, allow)

    def search_codes_dev(self, codes, k: int, allow=None):
        """``search`` with a uint8 torch tensor ``[nq, d / 8]`` on the store's device (``css_bin_search_codes_dev``)."""
        import torch

        dev = self._tensor(codes, torch.uint8, self.code_size, "search_codes_dev", 1)
        return self._search_dev(nat.lib().css_bin_search_codes_dev, codes, dev, k, allow)

    # ---- asymmetric searches: the query keeps its magnitudes at int8, the rows stay bits
    def _queries_i8(self, q8, what: str) -> np.ndarray:
        a = np.ascontiguousarray(q8)
        if a.dtype != np.int8 or a.ndim != 2 or a.shape[1] != self.d:
            raise ValueError(f"{what}: queries must be int8 [nq, {self.d}], got {a.dtype} {a.shape}")
        return a

    def search_asym(self, q8, k: int, allow=None) -> Tuple[np.ndarray, np.ndarray]:
        """``(D int32, I int64)``, each ``[nq, k]``: the ``k`` rows with the largest ``sum_i q8_i (2 b_i - 1)`` for each
        int8 query ``[nq, d]`` (every int8 value allowed), largest first, ties to the lower id; ``allow`` as in
        ``search``.  Padding: ``INT32_MIN`` / ``-1``.  ``1 <= k <= 128``."""
        return self._search_host(nat.lib().css_bin_search_asym_i8, self._queries_i8(q8, "search_asym"), k, allow)

    def search_asym_float(self, q, k: int, allow=None) -> Tuple[np.ndarray, np.ndarray]:
        """``search_asym`` of float32 queries ``[nq, d]``, quantized on the device as ``quantize_queries_numpy`` does."""
        return self._search_host(nat.lib().css_bin_search_asym, self._rows(q, "search_asym_float"), k, allow)

    def search_asym_dev(self, q, k: int, allow=None):
        """``search_asym_float`` with a float32 torch tensor ``[nq, d]`` on the store's device, enqueued on torch's
        current stream (``css_bin_search_asym_dev``): ``(D, I)`` as torch tensors there, the bytes of the host form."""
        import torch

        dev = self._tensor(q, torch.float32, self.d, "search_asym_dev", 1)
        return self._search_dev(nat.lib().css_bin_search_asym_dev, q, dev, k, allow)

    def search_asym_i8_dev(self, q8, k: int, allow=None):
        """``search_asym`` with an int8 torch tensor ``[nq, d]`` on the store's device (``css_bin_search_asym_i8_dev``)."""
        import torch

        dev = self._tensor(q8, torch.int8, self.d, "search_asym_i8_dev", 1)
        return self._search_dev(nat.lib().css_bin_search_asym_i8_dev, q8, dev, k, allow)
