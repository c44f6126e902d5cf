"""MUVERA fixed-dimensional encodings (Dhulipala et al., 2024): a token matrix ``[m, P]`` becomes ONE float32 row whose
inner product with a query's row estimates the MaxSim (Chamfer) score, so that the first stage of a late-interaction
search is the ordinary dense search and the second the exact MaxSim re-rank (``IndexFlat.add_fde`` / ``search_fde``).

``fde_numpy`` restates the definition of ``include/css_hip.h`` in float64 and is its documentation;
``FixedDimensionalEncoding`` runs it on the GPU (``css_fde_encode``, kernels in ``csrc/css_fde.h``)."""
from __future__ import annotations

import ctypes
from typing import Optional

import numpy as np

from . import _native as nat
from .flat_index import _bf16_bits, tokens_as_csr
from .late_interaction import bf16_to_f32, f32_to_bf16

MAX_KSIM = 6     # include/css_hip.h CSS_FDE_MAX_KSIM
MAX_REPS = 64    # include/css_hip.h CSS_FDE_MAX_REPS
MAX_DIM = 8192   # css_index_create's limit on d


def fde_args(P: int, k_sim: int, d_proj: int, reps: int) -> int:
    """The checked parameters; returns ``dim = reps * 2^k_sim * d_proj``.  What the library would refuse raises here."""
    if not (32 <= P <= nat.MAX_TOKEN_DIM and P % 32 == 0):
        raise ValueError(f"fde: P={P} must be a multiple of 32 in [32, {nat.MAX_TOKEN_DIM}]")
    if not 1 <= k_sim <= MAX_KSIM:
        raise ValueError(f"fde: k_sim={k_sim} outside [1, {MAX_KSIM}]")
    if d_proj not in (16, 32, 64):
        raise ValueError(f"fde: d_proj={d_proj} is not 16, 32 or 64")
    if not 1 <= reps <= MAX_REPS:
        raise ValueError(f"fde: reps={reps} outside [1, {MAX_REPS}]")
    dim = reps * (1 << k_sim) * d_proj
    if dim > MAX_DIM:
        raise ValueError(f"fde: dim = reps * 2^k_sim * d_proj = {dim} exceeds {MAX_DIM}")
    return dim


def default_material(P: int, k_sim: int, d_proj: int, reps: int, seed: int = 0):
    """``(planes uint16 [reps * k_sim, P], proj uint16 [reps * d_proj, P])`` as bf16 bits from
    ``numpy.random.default_rng(seed)``: standard normal planes rounded to bf16, ``proj = +-bf16(1 / sqrt(d_proj))``."""
    rng = np.random.default_rng(seed)
    planes = f32_to_bf16(rng.standard_normal((reps * k_sim, P)).astype(np.float32))
    s = bf16_to_f32(f32_to_bf16(np.float32(1.0 / np.sqrt(d_proj)).reshape(1)))[0]
    sign = rng.integers(0, 2, size=(reps * d_proj, P)) * 2 - 1
    return planes, f32_to_bf16((sign * s).astype(np.float32))


def fde_numpy(planes, proj, k_sim: int, d_proj: int, offsets, tok, is_query: bool, buckets=None):
    """The encoding in float64: ``(out float64 [n, dim], buckets uint8 [E, reps])``.  ``planes`` / ``proj`` / ``tok`` are
    bf16 bits (uint16) or floats, ``offsets`` int64 ``[n + 1]`` from 0.  ``buckets`` imposes an assignment (the
    device's, when the sums are checked apart from the sketch); otherwise bit i of ``bucket(t, r)`` is
    ``dot(x_t, planes[r * k_sim + i]) > 0``.  Documents: an empty bucket takes the token of least Hamming distance
    between bucket numbers, ties to the lowest token, and every bucket is divided by its count; queries: neither."""
    as64 = lambda a: (bf16_to_f32(a) if np.asarray(a).dtype == np.uint16 else np.asarray(a)).astype(np.float64)
    planes, proj, tok = as64(planes), as64(proj), as64(tok)
    off = np.asarray(offsets, dtype=np.int64)
    P = planes.shape[1]
    tok = tok.reshape(-1, P)
    reps, B, n = planes.shape[0] // k_sim, 1 << k_sim, off.shape[0] - 1
    if buckets is None:
        bits = (tok @ planes.T > 0).reshape(-1, reps, k_sim)
        buckets = (bits << np.arange(k_sim)).sum(axis=2)
    buckets = np.asarray(buckets).reshape(-1, reps).astype(np.uint8)
    out = np.zeros((n, reps, B, d_proj), dtype=np.float64)
    for i in range(n):
        x, bk = tok[off[i]:off[i + 1]], buckets[off[i]:off[i + 1]].astype(np.int64)
        if x.shape[0] == 0:
            continue
        for r in range(reps):
            onehot = bk[:, r, None] == np.arange(B)[None, :]          # [m, B]
            cnt = onehot.sum(axis=0)
            Y = onehot.T.astype(np.float64) @ x                        # [B, P]
            if not is_query:
                for b in np.flatnonzero(cnt == 0):
                    ham = np.array([bin(int(v) ^ int(b)).count("1") for v in bk[:, r]])
                    Y[b] = x[int(ham.argmin())]                        # (argmin: the first of equals)
                cnt = np.maximum(cnt, 1)
            o = Y @ proj[r * d_proj:(r + 1) * d_proj].T                # [B, d_proj]
            out[i, r] = o if is_query else o / cnt[:, None]
    return out.reshape(n, reps * B * d_proj), buckets


class FixedDimensionalEncoding:
    """The encoder on the GPU.  ``planes`` / ``proj`` (bf16 bits, or bf16-exact float32) replace the default material of
    ``default_material(P, k_sim, d_proj, reps, seed)``.  ``mats`` is whatever ``tokens_as_csr`` takes; a query matrix
    may hold up to 512 tokens here (the 64-token limit belongs to the MaxSim kernels)."""

    def __init__(self, P: int, k_sim: int = 5, d_proj: int = 16, reps: int = 16, seed: int = 0, device: int = 0,
                 planes=None, proj=None):
        self.P, self.k_sim, self.d_proj, self.reps, self.device = int(P), int(k_sim), int(d_proj), int(reps), int(device)
        self.dim = fde_args(self.P, self.k_sim, self.d_proj, self.reps)
        if planes is None or proj is None:   # (one draw: the default planes and proj come from the same stream)
            dp, dj = default_material(self.P, self.k_sim, self.d_proj, self.reps, seed)
        self.planes = dp if planes is None else np.ascontiguousarray(_bf16_bits(planes, "fde", "planes"))
        self.proj = dj if proj is None else np.ascontiguousarray(_bf16_bits(proj, "fde", "proj"))
        for a, rows, name in ((self.planes, self.reps * self.k_sim, "planes"), (self.proj, self.reps * self.d_proj, "proj")):
            if a.shape != (rows, self.P):
                raise ValueError(f"fde: {name} has shape {a.shape}, not {(rows, self.P)}")
            if ((a & 0x7F80) == 0x7F80).any():
                raise ValueError(f"fde: {name} holds a NaN or infinite component")
        self._h: Optional[ctypes.c_void_p] = None
        h = ctypes.c_void_p()
        nat.check(nat.lib().css_fde_create(self.P, self.k_sim, self.d_proj, self.reps, self.planes.ctypes.data,
                                           self.proj.ctypes.data, self.device, ctypes.byref(h)))
        self._h = h

    def close(self) -> None:
        if getattr(self, "_h", None) is not None:
            nat.lib().css_fde_free(self._h)
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
            raise RuntimeError("the encoder has been freed")
        return self._h

    def _csr(self, mats, keep, what):
        off, tok, P = tokens_as_csr(mats, keep, what)
        if tok.shape[0] and P != self.P:
            raise ValueError(f"{what}: the matrices have P={P}, the encoder P={self.P}")
        return off, tok

    def _encode(self, mats, keep, is_query: bool, with_buckets: bool, what: str):
        off, tok = self._csr(mats, keep, what)
        n = off.shape[0] - 1
        out = np.zeros((n, self.dim), dtype=np.float32)
        bk = np.zeros((tok.shape[0], self.reps), dtype=np.uint8) if with_buckets else None
        if n:
            nat.check(nat.lib().css_fde_encode(self._handle(), off.ctypes.data, tok.ctypes.data if tok.size else None, n,
                                               1 if is_query else 0, out.ctypes.data,
                                               bk.ctypes.data if with_buckets and bk.size else None))
        return (out, bk) if with_buckets else out

    def encode_documents(self, mats, keep=None, with_buckets: bool = False):
        """float32 ``[n, dim]`` (``with_buckets``: and the bucket bytes ``[E, reps]``); ``keep`` drops tokens first."""
        return self._encode(mats, keep, False, with_buckets, "encode_documents")

    def encode_queries(self, mats, with_buckets: bool = False):
        return self._encode(mats, None, True, with_buckets, "encode_queries")

    def _encode_dev(self, mats, keep, is_query: bool, what: str):
        import torch

        off, tok = self._csr(mats, keep, what)
        n = off.shape[0] - 1
        dev = torch.device("cuda", self.device)
        out = torch.zeros((n, self.dim), dtype=torch.float32, device=dev)
        if n:
            off_d = torch.from_numpy(off).to(dev)
            tok_d = torch.from_numpy(tok.view(np.int16).reshape(-1)).to(dev)
            st = torch.cuda.current_stream(dev).cuda_stream
            nat.check(nat.lib().css_fde_encode_dev(self._handle(), off_d.data_ptr(), tok_d.data_ptr() if tok.size else None,
                                                   n, tok.shape[0], 1 if is_query else 0, out.data_ptr(), None,
                                                   ctypes.c_void_p(st)))
            # (off_d / tok_d are torch's: the caching allocator keeps them for this stream until the kernel is done)
        return out

    def encode_documents_dev(self, mats, keep=None):
        """``encode_documents`` into a torch tensor ``[n, dim]`` on the encoder's device, enqueued on torch's current
        stream (``css_fde_encode_dev``): the bytes of the host form."""
        return self._encode_dev(mats, keep, False, "encode_documents_dev")

    def encode_queries_dev(self, mats):
        """``encode_queries`` into a torch tensor on the encoder's device, as ``encode_documents_dev``."""
        return self._encode_dev(mats, None, True, "encode_queries_dev")
