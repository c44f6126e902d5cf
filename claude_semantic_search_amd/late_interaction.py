"""``LateInteraction``: ColBERT-style re-ranking on the GPU encoder, in the shape of ``CrossEncoder`` (``predict`` /
``rank``).

Query and text are encoded APART, as in a bi-encoder, but keep one unit vector per token; the score of a pair is
``sum over query tokens s of max over kept text tokens t of dot(q_s, d_t)`` (MaxSim).  The text side does not depend on
the query: ``encode_documents`` forms token matrices once, ``score`` re-ranks kept matrices with one small kernel and no
forward pass (``css_encoder_maxsim``); ``predict`` / ``rank`` send uncached texts through ``css_encoder_forward_maxsim``.

A checkpoint is ``BertModel`` plus one bias-free ``linear.weight [P, H]`` (the colbert-ir layout: ``config.json`` of a
BERT model, weights under ``bert.*``); a directory without ``linear.weight`` uses the hidden states themselves (P = H).
Token matrices are uint16 arrays of bf16 bit patterns, as the device writes them.
"""
from __future__ import annotations

from pathlib import Path
from typing import Dict, List, Optional, Sequence, Tuple, Union

import numpy as np

from . import synth
from .cross_encoder import rank_scores
from .mpnet_encoder import BERT_SMALL_CFG, MpnetEncoder, _find_model_dir, _load_state_dict, parse_model_config

#: synthetic tensor id and std of the token projection (the body uses 0-5 and 16 + 16 * layer + 0..15, the
#: cross-encoder head 6-9)
PROJ_SYNTH = (10, 0.05)
MAX_QUERY_TOKENS = 64
_PROJ_KEY = "linear.weight"


def bf16_to_f32(m: np.ndarray) -> np.ndarray:
    """float32 values of a uint16 array of bf16 bit patterns."""
    return (np.asarray(m, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32)


def f32_to_bf16(x: np.ndarray) -> np.ndarray:
    """uint16 bf16 bit patterns of float32 values, round to nearest even (finite inputs)."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def maxsim_numpy(q, d, keep=None) -> float:
    """The MaxSim score in float64: ``sum_s max_{t: keep[t]} dot(q[s], d[t])`` over float (or bf16 uint16) matrices
    ``q`` [mq, P] and ``d`` [md, P].  Restates the device's score for the host tests and the fakes."""
    q = bf16_to_f32(q) if np.asarray(q).dtype == np.uint16 else np.asarray(q)
    d = bf16_to_f32(d) if np.asarray(d).dtype == np.uint16 else np.asarray(d)
    sim = q.astype(np.float64) @ d.astype(np.float64).T
    if keep is not None:
        k = np.asarray(keep).reshape(-1) != 0
        if k.size != d.shape[0]:
            raise ValueError(f"maxsim_numpy: {k.size} keep flags for {d.shape[0]} doc tokens")
        if not k.any():
            raise ValueError("maxsim_numpy: the doc has no kept token")
        sim = sim[:, k]
    return float(sim.max(axis=1).sum())


def build_side(ids: Sequence[int], marker_id: Optional[int], max_length: int) -> List[int]:
    """``[CLS] marker w.. [SEP]`` from the tokenizer's ``[CLS] w.. [SEP]``, cut to ``max_length`` tokens: the marker
    goes after ``[CLS]`` (``None``: no marker), and a cut drops the last words, never ``[CLS]``, the marker or the
    final ``[SEP]``."""
    ids = [int(t) for t in ids]
    floor = 2 if marker_id is None else 3
    if max_length < floor:
        raise ValueError(f"build_side: max_length={max_length} leaves no room for [CLS]{'' if marker_id is None else ' marker'} [SEP]")
    if marker_id is not None:
        ids = ids[:1] + [int(marker_id)] + ids[1:]
    if len(ids) > max_length:
        ids = ids[:max_length - 1] + ids[-1:]
    return ids


def keep_flags(ids: Sequence[int], skip_ids) -> np.ndarray:
    """uint8 flag per token: 0 for the ids in ``skip_ids`` (ColBERT's punctuation skiplist), 1 otherwise."""
    a = np.asarray(list(ids), dtype=np.int64)
    return (~np.isin(a, np.asarray(sorted(skip_ids), dtype=np.int64))).astype(np.uint8)


def parse_late_interaction_config(model_dir: Union[str, Path]) -> dict:
    """The encoder configuration of a ColBERT checkpoint directory (no GPU needed).  Refuses, with a ``ValueError``
    naming the field: a ``model_type`` other than ``bert`` and whatever ``parse_model_config`` refuses."""
    import json

    hf = json.loads((Path(model_dir) / "config.json").read_text())
    if hf.get("model_type") != "bert":
        raise ValueError(f"unsupported model_type {hf.get('model_type')!r} for a late-interaction checkpoint "
                         "(supported: 'bert')")
    cfg = parse_model_config(model_dir)
    cfg.update(pooling="cls", normalize=True)
    return cfg


def split_projection(sd: Dict[str, np.ndarray], hidden: int) -> Tuple[Dict[str, np.ndarray], Optional[np.ndarray]]:
    """``(body, W)`` of a colbert-ir state dict: ``linear.weight`` [P, H] is the token projection (``None`` when the
    checkpoint has none), everything else the ``BertModel`` body.  Refuses a ``linear.bias`` (ColBERT's projection has
    none) and a projection whose shape the kernels do not run, naming the tensor."""
    if "linear.bias" in sd:
        raise ValueError("unsupported linear.bias: the token projection of a late-interaction checkpoint is bias-free")
    body = {k: v for k, v in sd.items() if k != _PROJ_KEY}
    W = sd.get(_PROJ_KEY)
    if W is not None:
        W = np.asarray(W, dtype=np.float32)
        if W.ndim != 2 or W.shape[1] != hidden or W.shape[0] % 32 or not 32 <= W.shape[0] <= 128:
            raise ValueError(f"unsupported linear.weight of shape {W.shape}: expected [P, {hidden}] with P a multiple "
                             "of 32 in [32, 128]")
    return body, W


def synth_projection(hidden: int, dim: int, seed: int) -> np.ndarray:
    """The seeded synthetic projection [dim, hidden], N(0, 0.05^2), formed on the host with ``synth``."""
    tid, std = PROJ_SYNTH
    v = synth.normal(synth.tensor_seed(seed, tid), np.arange(dim * hidden, dtype=np.uint64))
    return (np.float32(std) * v).astype(np.float32).reshape(dim, hidden)


class LateInteraction:
    def __init__(self, model_name_or_path: Optional[str], device: int = 0, compute: str = "bf16",
                 synthetic_seed: Optional[int] = None, cfg_overrides: Optional[dict] = None, query_length: int = 32,
                 document_length: Optional[int] = None, query_marker_id: Optional[int] = 1,
                 document_marker_id: Optional[int] = 2, skip_ids: Sequence[int] = (), projection_dim: Optional[int] = 128,
                 encoder=None):
        # encoder: an object with the late-interaction surface of MpnetEncoder (tests pass a fake; no GPU is touched)
        self.model_dir = None
        self._owns_encoder = encoder is None      # a caller's encoder stays the caller's: close() leaves it open
        if encoder is not None:
            self.encoder = encoder
        elif synthetic_seed is None:
            model_dir = _find_model_dir(model_name_or_path or "", None)
            if model_dir is None:
                raise FileNotFoundError(f"model '{model_name_or_path}' not found locally (no network): pass a directory "
                                        "in HF layout, or synthetic_seed=<int> for seeded synthetic weights")
            cfg = parse_late_interaction_config(model_dir)
            body, W = split_projection(_load_state_dict(model_dir), int(cfg["hidden"]))
            over = dict(pooling=cfg["pooling"], normalize=cfg["normalize"])
            over.update(cfg_overrides or {})
            self.encoder = MpnetEncoder(str(model_dir), device=device, compute=compute, cfg_overrides=over, weights=body)
            try:
                self.encoder.set_token_projection(W)
                if self.encoder.tokenizer is None:
                    raise FileNotFoundError(self.encoder.tokenizer_problem)
            except Exception:
                self.encoder.close()
                raise
            self.model_dir = model_dir
        else:
            cfg = dict(BERT_SMALL_CFG, pooling="cls", normalize=True)
            if cfg_overrides:
                cfg.update(cfg_overrides)
            if cfg.get("arch") != "bert":
                raise ValueError(f"unsupported arch {cfg.get('arch')!r} for late interaction (supported: 'bert')")
            self.encoder = MpnetEncoder(synthetic_seed=synthetic_seed, device=device, compute=compute, cfg_overrides=cfg)
            if projection_dim:
                try:
                    self.encoder.set_token_projection(synth_projection(int(cfg["hidden"]), int(projection_dim), synthetic_seed))
                except Exception:
                    self.encoder.close()
                    raise
        self.cfg = self.encoder.cfg
        self.tokenizer = self.encoder.tokenizer
        limit = int(self.cfg["max_seq_len"])
        self.query_length = int(query_length)
        self.document_length = limit if document_length is None else int(document_length)
        self.query_marker_id, self.document_marker_id = query_marker_id, document_marker_id
        self.skip_ids = frozenset(int(t) for t in skip_ids)
        problem = None
        if not 3 <= self.query_length <= min(MAX_QUERY_TOKENS, limit):
            problem = f"query_length={self.query_length} outside [3, {min(MAX_QUERY_TOKENS, limit)}]"
        elif not 3 <= self.document_length <= limit:
            problem = f"document_length={self.document_length} outside [3, {limit}] (the encoder's max_seq_len)"
        else:
            for name, m in (("query_marker_id", query_marker_id), ("document_marker_id", document_marker_id)):
                if m is not None and (not 0 <= int(m) < int(self.cfg["vocab"]) or int(m) == int(self.cfg["pad_id"])):
                    problem = f"{name}={m} is outside the vocabulary or the pad id"
        if problem:
            self.close()
            raise ValueError(problem)

    def close(self) -> None:
        if self._owns_encoder:
            self.encoder.close()

    def __enter__(self) -> "LateInteraction":
        return self

    def __exit__(self, *exc) -> None:
        self.close()

    @property
    def token_dim(self) -> int:
        return int(self.encoder.token_dim)

    # -- ids --------------------------------------------------------------------
    def _side_ids(self, texts: Sequence[str], marker_id: Optional[int], max_length: int) -> List[List[int]]:
        return [build_side(t, marker_id, max_length) for t in self.encoder.tokenize(list(texts))]

    def query_ids(self, texts: Sequence[str]) -> List[List[int]]:
        """``[CLS] [Q] w.. [SEP]`` per text, at most ``query_length`` tokens (longer queries are cut)."""
        return self._side_ids(texts, self.query_marker_id, self.query_length)

    def document_ids(self, texts: Sequence[str]) -> List[List[int]]:
        """``[CLS] [D] w.. [SEP]`` per text, at most ``document_length`` tokens."""
        return self._side_ids(texts, self.document_marker_id, self.document_length)

    def _keep(self, ids: List[List[int]]) -> Optional[List[np.ndarray]]:
        return [keep_flags(s, self.skip_ids) for s in ids] if self.skip_ids else None

    # -- token matrices -----------------------------------------------------------
    def _encode(self, ids: List[List[int]], batch_size: int) -> List[np.ndarray]:
        mats: List[Optional[np.ndarray]] = [None] * len(ids)
        bs = max(1, int(batch_size))
        order = sorted(range(len(ids)), key=lambda i: -len(ids[i]))
        for s in range(0, len(order), bs):
            idx = order[s:s + bs]
            for i, m in zip(idx, self.encoder.encode_tokens_ids([ids[i] for i in idx], normalize=True)):
                mats[i] = np.array(m, copy=True)
        return mats

    def encode_queries(self, texts: Sequence[str], batch_size: int = 32):
        """``(mats, keep)``: per query its unit token matrix (uint16 [m, P] of bf16 bits); ``keep`` is ``None`` (the
        skiplist applies to the document side only)."""
        return self._encode(self.query_ids(texts), batch_size), None

    def encode_documents(self, texts: Sequence[str], batch_size: int = 32):
        """``(mats, keep)``: per text its unit token matrix and, with ``skip_ids``, one flag per token (else ``None``).
        Both can be kept and scored later with ``score``: no forward pass then."""
        ids = self.document_ids(texts)
        return self._encode(ids, batch_size), self._keep(ids)

    def score(self, q_mats, d_mats, pairs=None, keep=None) -> np.ndarray:
        """float32 MaxSim scores of kept token matrices, one per ``(query, doc)`` pair (``None``: all, query-major)."""
        return self.encoder.maxsim(q_mats, d_mats, pairs=pairs, keep=keep)

    # -- CrossEncoder surface -------------------------------------------------------
    def predict(self, pairs: Sequence[Sequence[str]], batch_size: int = 32, activation: Optional[str] = None) -> np.ndarray:
        """float32 MaxSim scores, one per ``(query, text)`` pair, in input order.  Every distinct query text is encoded
        once; the texts go through ``css_encoder_forward_maxsim`` in length-sorted batches, so nothing per token leaves
        the device.  ``activation`` must be ``None`` (a MaxSim score is no logit)."""
        if activation is not None:
            raise ValueError(f"unsupported activation {activation!r} (supported: None)")
        pairs = list(pairs)
        if not pairs:
            return np.zeros(0, dtype=np.float32)
        qtexts: List[str] = []
        qindex: Dict[str, int] = {}
        for p in pairs:
            if p[0] not in qindex:
                qindex[p[0]] = len(qtexts)
                qtexts.append(p[0])
        q_mats, _ = self.encode_queries(qtexts, batch_size)
        ids = self.document_ids([p[1] for p in pairs])
        keep = self._keep(ids)
        out = np.empty(len(pairs), dtype=np.float32)
        bs = max(1, int(batch_size))
        order = sorted(range(len(ids)), key=lambda i: -len(ids[i]))
        for s in range(0, len(order), bs):
            idx = order[s:s + bs]
            used = sorted({qindex[pairs[i][0]] for i in idx})
            local = {q: n for n, q in enumerate(used)}
            pr = [(local[qindex[pairs[i][0]]], n) for n, i in enumerate(idx)]
            out[idx] = self.encoder.score_late_ids([ids[i] for i in idx], [q_mats[q] for q in used], pairs=pr,
                                                   keep=[keep[i] for i in idx] if keep is not None else None)
        return out

    def rank(self, query: str, documents: Sequence[str], top_k: Optional[int] = None,
             return_documents: bool = False) -> List[dict]:
        """``[{"corpus_id", "score"[, "text"]}]`` of ``documents`` against ``query``, best first; ties go to the lower
        ``corpus_id``."""
        documents = list(documents)
        return rank_scores(self.predict([(query, d) for d in documents]), documents, top_k, return_documents)
