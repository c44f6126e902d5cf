"""The scalar-quantized row store (``faiss.IndexScalarQuantizer`` ``QT_8bit`` / ``QT_4bit``; Lucene ``int8_flat`` /
``int4_flat``): a dense row of ``d`` components kept as ``d`` codes of 8 or 4 bits on a per-component grid
``vmin[i] + c step[i]`` and nothing else, scanned exhaustively.  The ranges fold into an int8 query, so the score
``sum_i q8_i c_i`` is an integer: ``include/css_hip.h`` defines codes, query and ranking in bits.

``ScalarQuantizer`` holds the ranges and restates the definition in numpy (the device's bytes); ``train_scalar_quantizer``
takes the ranges from a sample; ``IndexScalarQuantizer`` is the store on the GPU (``css_sq_*``, kernels in
``csrc/css_sq.h``)."""
from __future__ import annotations

import ctypes
from typing import Optional, Tuple

import numpy as np

from . import _native as nat
from . import binary
from .flat_index import pack_allow_bits

MAX_DIM = 8192        # css_sq_create's limit on d
MAX_K = 128           # the searches' limit on k
MAX_QUERIES = 65536   # include/css_hip.h CSS_BIN_MAX_QUERIES
MAX_WAVES = 16384     # include/css_hip.h CSS_BIN_MAX_WAVES
PAD_SCORE = np.iinfo(np.int32).min

search_numpy = binary.search_asym_numpy   # largest score first, ties to the lower id, padding INT32_MIN / -1


class ScalarQuantizer:
    """The grid: ``bits`` 4 or 8 (``L = 2^bits - 1`` levels above 0), float32 ``vmin[d]`` (finite) and ``step[d]``
    (finite, above 0).  What ``css_sq_create`` would refuse raises here."""

    def __init__(self, d: int, bits: int, vmin, step):
        self.d, self.bits = int(d), int(bits)
        if not (32 <= self.d <= MAX_DIM and self.d % 32 == 0):
            raise ValueError(f"sq: d={self.d} must be a multiple of 32 in [32, {MAX_DIM}]")
        if self.bits not in (4, 8):
            raise ValueError(f"sq: bits={self.bits} must be 4 or 8")
        self.L = (1 << self.bits) - 1
        self.code_size = self.d * self.bits // 8
        self.vmin = np.ascontiguousarray(vmin, dtype=np.float32)
        self.step = np.ascontiguousarray(step, dtype=np.float32)
        if self.vmin.shape != (self.d,) or self.step.shape != (self.d,):
            raise ValueError(f"sq: vmin and step must have shape ({self.d},), got {self.vmin.shape} and {self.step.shape}")
        if not np.isfinite(self.vmin).all():
            raise ValueError("sq: vmin holds a NaN or infinite component")
        if not (np.isfinite(self.step) & (self.step > 0)).all():
            raise ValueError("sq: every step must be finite and above 0")

    def _rows(self, x, what: str) -> np.ndarray:
        a = np.ascontiguousarray(x, dtype=np.float32)
        if a.ndim != 2 or a.shape[1] != self.d:
            raise ValueError(f"{what}: expected shape [n, {self.d}], got {a.shape}")
        if not np.isfinite(a).all():
            raise ValueError(f"{what}: a component is NaN or infinite")
        return a

    def _codes(self, codes, what: str) -> np.ndarray:
        c = np.ascontiguousarray(codes)
        if c.dtype != np.uint8 or c.ndim != 2 or c.shape[1] != self.code_size:
            raise ValueError(f"{what}: codes must be uint8 [n, {self.code_size}], got {c.dtype} {c.shape}")
        return c

    def levels(self, codes) -> np.ndarray:
        """The codes unpacked to one level per component: uint8 ``[n, d]`` (at 4 bits component ``2 j`` is the low
        nibble of byte ``j``)."""
        c = self._codes(codes, "levels")
        return c if self.bits == 8 else np.stack((c & 15, c >> 4), axis=-1).reshape(c.shape[0], self.d)

    def encode_numpy(self, x) -> np.ndarray:
        """``c_i = clamp(rint((x_i - vmin_i) / step_i), 0, L)`` in float32, one rounding per operation, ties to even;
        uint8 ``[n, d]`` at 8 bits, ``[n, d / 2]`` at 4."""
        a = self._rows(x, "encode_numpy")
        with np.errstate(over="ignore", under="ignore"):
            c = np.clip(np.rint((a - self.vmin) / self.step), 0, self.L).astype(np.uint8)
        return c if self.bits == 8 else c[:, 0::2] | c[:, 1::2] << 4

    def decode_numpy(self, codes) -> np.ndarray:
        """``fma(c_i, step_i, vmin_i)`` with ONE rounding to float32: ``[n, d]``.  The product is exact in float64; the
        sum's rounding error (TwoSum) decides the cases in which the float64 sum lies midway between two float32."""
        p = self.levels(codes).astype(np.float64) * self.step.astype(np.float64)
        v = np.broadcast_to(self.vmin.astype(np.float64), p.shape)
        s = p + v
        t = s - p
        err = (p - (s - t)) + (v - t)
        r = s.astype(np.float32)
        up = s > r   # the float32 neighbours a < s < b of a sum that is not a float32 itself
        a = np.where(up, r, np.nextafter(r, np.float32(-np.inf)))
        b = np.where(up, np.nextafter(r, np.float32(np.inf)), r)
        midway = (s != r) & (err != 0) & (a.astype(np.float64) / 2 + b.astype(np.float64) / 2 == s)
        return np.where(midway, np.where(err > 0, b, a), r).astype(np.float32)

    def quantize_queries_numpy(self, q) -> Tuple[np.ndarray, np.ndarray]:
        """The int8 form of float queries ``[nq, d]`` as ``search`` makes it: ``w_i = q_i step_i`` in float32, then the
        rule of ``binary.quantize_queries_numpy`` on ``w``.  Returns ``(q8 int8 [nq, d], a = max |w_i| float32 [nq])``."""
        with np.errstate(over="ignore", under="ignore"):
            w = self._rows(q, "quantize_queries_numpy") * self.step
        if not np.isfinite(w).all():
            raise ValueError("quantize_queries_numpy: a component times its step is infinite")
        return binary.quantize_queries_numpy(w)

    def scores_numpy(self, q8, codes) -> np.ndarray:
        """``sum_i q8_i c_i`` of int8 queries ``[nq, d]`` against codes: int64 ``[nq, n]`` (below 2^28: exact in float64,
        1024 rows at a time)."""
        qf, lv = np.asarray(q8, dtype=np.int8).astype(np.float64), self.levels(codes)
        parts = [qf @ lv[r:r + 1024].astype(np.float64).T for r in range(0, lv.shape[0], 1024)]
        return np.concatenate(parts, axis=1).astype(np.int64) if parts else np.zeros((qf.shape[0], 0), dtype=np.int64)

    def estimate(self, q, D) -> np.ndarray:
        """The float64 estimate ``sum_i q_i vmin_i + a s / 127`` of ``<q, decode(r)>`` from the scores ``D [nq, k]`` of
        ``search(q, k)``; ``-inf`` where ``D`` is padding."""
        a = self.quantize_queries_numpy(q)[1].astype(np.float64)
        base = self._rows(q, "estimate").astype(np.float64) @ self.vmin.astype(np.float64)
        D = np.asarray(D)
        return np.where(D == PAD_SCORE, -np.inf, base[:, None] + a[:, None] * D.astype(np.float64) / 127)


def train_scalar_quantizer(sample, bits: int, quantile: float = 1.0) -> ScalarQuantizer:
    """The ranges from a sample ``[n, d]``, on the host: per component ``vmin`` and ``vmax`` are the ``1 - quantile`` and
    ``quantile`` quantiles (1.0: minimum and maximum), ``step = (vmax - vmin) / L``; a constant component gets a step
    of 1."""
    x = np.asarray(sample, dtype=np.float32)
    if x.ndim != 2 or x.shape[0] == 0 or not np.isfinite(x).all():
        raise ValueError("train_scalar_quantizer: the sample must be a non-empty finite [n, d]")
    if not 0.5 < quantile <= 1.0:
        raise ValueError(f"train_scalar_quantizer: quantile={quantile} outside (0.5, 1]")
    lo, hi = np.quantile(x.astype(np.float64), (1.0 - quantile, quantile), axis=0)
    step = ((hi - lo) / ((1 << int(bits)) - 1)).astype(np.float32)
    step[~(np.isfinite(step) & (step > 0))] = 1.0
    return ScalarQuantizer(x.shape[1], bits, lo.astype(np.float32), step)


class IndexScalarQuantizer:
    """The store on the GPU over a ``ScalarQuantizer``.  Rows are numbered in the order they were added; nothing but
    their codes is kept."""

    def __init__(self, sq: ScalarQuantizer, device: int = 0):
        self._h: Optional[ctypes.c_void_p] = None
        self.sq, self.d, self.bits, self.code_size, self.device = sq, sq.d, sq.bits, sq.code_size, int(device)
        h = ctypes.c_void_p()
        nat.check(nat.lib().css_sq_create(self.d, self.bits, sq.vmin.ctypes.data, sq.step.ctypes.data, self.device, ctypes.byref(h)))
        self._h = h

    def close(self) -> None:
        if getattr(self, "_h", None) is not None:
            nat.lib().css_sq_free(self._h)
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
        nat.check(nat.lib().css_sq_ntotal(self._handle(), ctypes.byref(n)))
        return int(n.value)

    @property
    def last_passes(self) -> int:
        """The scans of the codes the last search made: ``ceil(nq / 16)``."""
        p = ctypes.c_int(0)
        nat.check(nat.lib().css_sq_last_passes(self._handle(), ctypes.byref(p)))
        return int(p.value)

    def set_waves(self, waves: int) -> None:
        """The number of scanning waves (row ranges) of the next searches, 0 = automatic.  No answer depends on it."""
        waves = int(waves)
        if not 0 <= waves <= MAX_WAVES:
            raise ValueError(f"set_waves: waves={waves} outside [0, {MAX_WAVES}]")
        nat.check(nat.lib().css_sq_set_waves(self._handle(), waves))

    def _tensor(self, t, dtype, what: str, min_rows: int):
        import torch

        if t.dtype != dtype or t.dim() != 2 or t.shape[1] != self.d or not t.is_contiguous() or t.shape[0] < min_rows:
            raise ValueError(f"{what}: expected a contiguous {dtype} tensor [n >= {min_rows}, {self.d}]")
        dev = torch.device("cuda", self.device)
        if t.device != dev:
            raise ValueError(f"{what}: the tensor is on {t.device}, the store on device {self.device}")
        return dev

    # ---- rows
    def add(self, x) -> None:
        """Encode float32 rows ``[n, d]`` on the device and append their codes."""
        a = self.sq._rows(x, "add")
        if a.shape[0]:
            nat.check(nat.lib().css_sq_add(self._handle(), a.ctypes.data, a.shape[0]))

    def add_dev(self, x) -> None:
        """``add`` from a contiguous float32 torch tensor ``[n, d]`` on the store's device, enqueued on torch's current
        stream (``css_sq_add_dev``).  The contents are not checked."""
        import torch

        dev = self._tensor(x, torch.float32, "add_dev", 0)
        if x.shape[0]:
            st = torch.cuda.current_stream(dev).cuda_stream
            nat.check(nat.lib().css_sq_add_dev(self._handle(), x.data_ptr(), x.shape[0], ctypes.c_void_p(st)))

    def add_codes(self, codes) -> None:
        """Append rows that are codes: uint8 ``[n, d]`` (8 bits) or ``[n, d / 2]`` (4 bits, low nibble first)."""
        c = self.sq._codes(codes, "add_codes")
        if c.shape[0]:
            nat.check(nat.lib().css_sq_add_codes(self._handle(), c.ctypes.data, c.shape[0]))

    def _read(self, fn, row0: int, n: Optional[int], width: int, dtype) -> np.ndarray:
        row0 = int(row0)
        n = self.ntotal - row0 if n is None else int(n)
        out = np.empty((max(n, 0), width), dtype=dtype)
        nat.check(fn(self._handle(), row0, n, out.ctypes.data))
        return out

    def get_codes(self, row0: int = 0, n: Optional[int] = None) -> np.ndarray:
        """The codes of rows ``[row0, row0 + n)``, the form ``add_codes`` takes."""
        return self._read(nat.lib().css_sq_get_codes, row0, n, self.code_size, np.uint8)

    def reconstruct_n(self, row0: int = 0, n: Optional[int] = None) -> np.ndarray:
        """Rows ``[row0, row0 + n)`` decoded on the device: float32 ``[n, d]``, the bytes of ``decode_numpy``."""
        return self._read(nat.lib().css_sq_reconstruct, row0, n, self.d, np.float32)

    # ---- searches
    def _search_args(self, nq: int, k: int) -> int:
        k = int(k)
        if not 1 <= k <= MAX_K:
            raise ValueError(f"search: k={k} outside [1, {MAX_K}]")
        if nq > MAX_QUERIES:
            raise ValueError(f"search: nq={nq} exceeds {MAX_QUERIES}")
        return k

    def _queries_i8(self, q8, what: str) -> np.ndarray:
        a = np.ascontiguousarray(q8)
        if a.dtype != np.int8 or a.ndim != 2 or a.shape[1] != self.d:
            raise ValueError(f"{what}: queries must be int8 [nq, {self.d}], got {a.dtype} {a.shape}")
        return a

    def _search_host(self, fn, a: np.ndarray, k: int, allow) -> Tuple[np.ndarray, np.ndarray]:
        k = self._search_args(a.shape[0], k)
        D, I = np.empty((a.shape[0], k), dtype=np.int32), np.empty((a.shape[0], k), dtype=np.int64)
        bits = None if allow is None else pack_allow_bits(allow, self.ntotal)
        if a.shape[0]:
            nat.check(fn(self._handle(), a.ctypes.data, a.shape[0], k, None if bits is None else bits.ctypes.data,
                         D.ctypes.data, I.ctypes.data))
        return D, I

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

    def search(self, q, k: int, allow=None) -> Tuple[np.ndarray, np.ndarray]:
        """``(D int32, I int64)``, each ``[nq, k]``: for each float32 query ``[nq, d]``, folded and quantized on the device
        as ``quantize_queries_numpy`` does, the ``k`` rows with the largest ``sum_i q8_i c_i``, largest first, ties to the
        lower id; ``allow`` is a boolean mask over the rows.  Padding: ``INT32_MIN`` / ``-1``.  ``1 <= k <= 128``.
        ``sq.estimate(q, D)`` turns the scores into float estimates of the inner products."""
        a = self.sq._rows(q, "search")
        with np.errstate(over="ignore", under="ignore"):
            if not np.isfinite(a * self.sq.step).all():
                raise ValueError("search: a component times its step is infinite")
        return self._search_host(nat.lib().css_sq_search, a, k, allow)

    def search_i8(self, q8, k: int, allow=None) -> Tuple[np.ndarray, np.ndarray]:
        """``search`` of int8 queries ``[nq, d]`` taken as they are (every int8 value allowed, no folding)."""
        return self._search_host(nat.lib().css_sq_search_i8, self._queries_i8(q8, "search_i8"), k, allow)

    def search_dev(self, q, k: int, allow=None):
        """``search`` with a float32 torch tensor ``[nq, d]`` on the store's device, enqueued on torch's current stream
        (``css_sq_search_dev``): ``(D, I)`` as torch tensors there, the bytes of the host form."""
        import torch

        return self._search_dev(nat.lib().css_sq_search_dev, q, self._tensor(q, torch.float32, "search_dev", 1), k, allow)

    def search_i8_dev(self, q8, k: int, allow=None):
        """``search_i8`` with an int8 torch tensor ``[nq, d]`` on the store's device (``css_sq_search_i8_dev``)."""
        import torch

        return self._search_dev(nat.lib().css_sq_search_i8_dev, q8, self._tensor(q8, torch.int8, "search_i8_dev", 1), k, allow)
