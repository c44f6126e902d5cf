"""``SparseEncoder``: learned sparse retrieval (SPLADE and its descendants) on the GPU encoder, in the shape of
``CrossEncoder`` and ``LateInteraction`` (``predict`` / ``rank``).

A checkpoint is a ``BertForMaskedLM``: the body that ``MpnetEncoder`` runs plus the masked-LM head
(``cls.predictions.*``).  A text's weight for vocabulary term ``v`` is ``max over its tokens t of
log(1 + relu(logit[t, v]))``: one coordinate per word, so a vector can be read (``decode``), and words the text implies
but does not contain get weight (``expansion``).  The device keeps the ``m`` heaviest terms per text
(``css_encoder_forward_sparse``); a pair's score is the dot product over the shared terms, summed on the host.
"""
from __future__ import annotations

import json
import math
from pathlib import Path
from typing import Dict, List, NamedTuple, Optional, Sequence, Tuple, Union

import numpy as np

from . import synth
from .cross_encoder import rank_scores
from .mpnet_encoder import BERT_SMALL_CFG, MpnetEncoder, _find_model_dir, _load_state_dict, parse_model_config

#: synthetic tensor id and std of the head's tensors (the body uses 0-5 and 16 + 16 * layer + 0..15, the cross-encoder
#: head 6-9, the token projection 10); the decoder is tied
MLM_SYNTH = {"dense_w": (11, 0.02), "dense_b": (12, 0.05), "ln_g": (13, 0.1), "ln_b": (14, 0.05), "decoder_b": (15, 0.05)}
#: mean of the synthetic decoder bias in units of 0.02 sqrt(H), the standard deviation of a random-weight logit: with a
#: zero bias the maximum over a text's tokens turns most of the vocabulary positive and nothing is sparse
SYNTH_BIAS_SIGMAS = -3.5
MAX_TERMS = 512
_HEAD = "cls.predictions."


class SparseVector(NamedTuple):
    """A text's heaviest vocabulary terms, best first (ties to the lower term id)."""
    terms: np.ndarray     # int32 [n]
    weights: np.ndarray   # float32 [n]


def sparse_dot_numpy(q: SparseVector, d: SparseVector) -> np.float32:
    """The dot product over the shared terms: products summed in float64 in ascending term order, rounded to fp32
    once.  Restates ``SparseEncoder.score`` for the host tests and the fakes."""
    _, qi, di = np.intersect1d(np.asarray(q.terms), np.asarray(d.terms), assume_unique=True, return_indices=True)
    prod = np.asarray(q.weights, dtype=np.float64)[qi] * np.asarray(d.weights, dtype=np.float64)[di]
    return np.float32(math.fsum(prod))


def parse_sparse_config(model_dir: Union[str, Path]) -> dict:
    """The encoder configuration of a masked-LM checkpoint directory (no GPU needed).  Refuses, with a ``ValueError``
    naming the field: a ``model_type`` other than ``bert`` and whatever ``parse_model_config`` refuses."""
    hf = json.loads((Path(model_dir) / "config.json").read_text())
    if hf.get("model_type") != "bert":
        raise ValueError(f"unsupported model_type {hf.get('model_type')!r} for a sparse encoder (supported: 'bert')")
    cfg = parse_model_config(model_dir)
    cfg.update(pooling="cls", normalize=False)
    return cfg


def split_mlm_head(sd: Dict[str, np.ndarray], hidden: int, vocab: int) -> Tuple[Dict[str, np.ndarray], Dict[str, Optional[np.ndarray]]]:
    """``(body, head)`` of a ``BertForMaskedLM`` state dict.  ``head`` has ``dense_w`` [H, H], ``dense_b`` [H], ``ln_g``,
    ``ln_b`` [H] (``cls.predictions.transform.{dense,LayerNorm}.{weight,bias}``), ``decoder_w`` [V, H]
    (``cls.predictions.decoder.weight``; ``None`` when the checkpoint leaves it out: a tied decoder) and ``decoder_b``
    [V] (``cls.predictions.bias`` and / or ``cls.predictions.decoder.bias``, which must be equal when both are there).
    Names may carry ``bert.``.  Refuses a missing tensor, a wrong shape and unequal biases, naming the tensor."""
    body: Dict[str, np.ndarray] = {}
    raw: Dict[str, np.ndarray] = {}
    for k, v in sd.items():
        name = k[5:] if k.startswith("bert.") else k
        if name.startswith(_HEAD):
            if name in raw:
                raise ValueError(f"masked-LM checkpoint names '{name}' more than once")
            raw[name] = np.asarray(v, dtype=np.float32)
        else:
            body[k] = v
    want = {"dense_w": ("transform.dense.weight", (hidden, hidden)), "dense_b": ("transform.dense.bias", (hidden,)),
            "ln_g": ("transform.LayerNorm.weight", (hidden,)), "ln_b": ("transform.LayerNorm.bias", (hidden,))}
    head: Dict[str, Optional[np.ndarray]] = {}

    def take(key: str, shape, required: bool) -> Optional[np.ndarray]:
        a = raw.pop(_HEAD + key, None)
        if a is None:
            if required:
                raise ValueError(f"checkpoint has no {_HEAD}{key}: a sentence encoder, not a masked-LM checkpoint "
                                 "(BertForMaskedLM keeps cls.predictions.*)")
            return None
        if a.shape != shape:
            raise ValueError(f"unsupported {_HEAD}{key} of shape {a.shape}: expected {shape}")
        return a

    for out, (key, shape) in want.items():
        head[out] = take(key, shape, True)
    head["decoder_w"] = take("decoder.weight", (vocab, hidden), False)
    b1, b2 = take("bias", (vocab,), False), take("decoder.bias", (vocab,), False)
    if b1 is None and b2 is None:
        raise ValueError(f"checkpoint has no {_HEAD}bias (nor {_HEAD}decoder.bias)")
    if b1 is not None and b2 is not None and not np.array_equal(b1, b2):
        raise ValueError(f"{_HEAD}bias and {_HEAD}decoder.bias differ: the decoder has one bias")
    head["decoder_b"] = b1 if b1 is not None else b2
    if raw:
        raise ValueError(f"unsupported tensor {sorted(raw)[0]} in the masked-LM head")
    return body, head


def synth_mlm_head(hidden: int, vocab: int, seed: int, bias_sigmas: float = SYNTH_BIAS_SIGMAS) -> Dict[str, Optional[np.ndarray]]:
    """The seeded synthetic head, formed on the host with ``synth`` (tensor ids ``MLM_SYNTH``): dense weight
    N(0, 0.02^2), dense bias N(0, 0.05^2), LayerNorm weight N(1, 0.1^2) and bias N(0, 0.05^2), a tied decoder
    (``decoder_w`` is ``None``) and the decoder bias N(bias_sigmas * 0.02 sqrt(hidden), 0.05^2)."""
    def t(key, n, mean=0.0):
        tid, std = MLM_SYNTH[key]
        v = synth.normal(synth.tensor_seed(seed, tid), np.arange(n, dtype=np.uint64))
        return (np.float32(mean) + np.float32(std) * v).astype(np.float32)

    return {"dense_w": t("dense_w", hidden * hidden).reshape(hidden, hidden), "dense_b": t("dense_b", hidden),
            "ln_g": t("ln_g", hidden, 1.0), "ln_b": t("ln_b", hidden), "decoder_w": None,
            "decoder_b": t("decoder_b", vocab, bias_sigmas * 0.02 * math.sqrt(hidden))}


class SparseEncoder:
    def __init__(self, model_name_or_path: Optional[str], device: int = 0, compute: str = "bf16",
                 max_length: Optional[int] = None, synthetic_seed: Optional[int] = None,
                 cfg_overrides: Optional[dict] = None, encoder=None):
        # encoder: an object with the sparse surface of MpnetEncoder (tests pass a fake; no GPU is touched)
        self.model_dir = None
        self._owns_encoder = encoder is None      # a caller's encoder stays the caller's: close() leaves it open
        if encoder is not None:
            self.encoder = encoder
        elif synthetic_seed is None:
            model_dir = _find_model_dir(model_name_or_path or "", None)
            if model_dir is None:
                raise FileNotFoundError(f"model '{model_name_or_path}' not found locally (no network): pass a directory "
                                        "in HF layout, or synthetic_seed=<int> for seeded synthetic weights")
            cfg = parse_sparse_config(model_dir)
            body, head = split_mlm_head(_load_state_dict(model_dir), int(cfg["hidden"]), int(cfg["vocab"]))
            over = dict(pooling=cfg["pooling"], normalize=cfg["normalize"])
            over.update(cfg_overrides or {})
            self.encoder = MpnetEncoder(str(model_dir), device=device, compute=compute, cfg_overrides=over, weights=body)
            try:
                self.encoder.set_mlm_head(**head)
                if self.encoder.tokenizer is None:
                    raise FileNotFoundError(self.encoder.tokenizer_problem)
            except Exception:
                self.encoder.close()
                raise
            self.model_dir = model_dir
        else:
            cfg = dict(BERT_SMALL_CFG, pooling="cls", normalize=False)
            if cfg_overrides:
                cfg.update(cfg_overrides)
            if cfg.get("arch") != "bert":
                raise ValueError(f"unsupported arch {cfg.get('arch')!r} for a sparse encoder (supported: 'bert')")
            self.encoder = MpnetEncoder(synthetic_seed=synthetic_seed, device=device, compute=compute, cfg_overrides=cfg)
            try:
                self.encoder.set_mlm_head(**synth_mlm_head(int(cfg["hidden"]), int(cfg["vocab"]), synthetic_seed))
            except Exception:
                self.encoder.close()
                raise
        self.cfg = self.encoder.cfg
        self.tokenizer = self.encoder.tokenizer
        limit = int(self.cfg["max_seq_len"])
        self.max_length = limit if max_length is None else int(max_length)
        if not 2 <= self.max_length <= limit:
            self.close()
            raise ValueError(f"max_length={self.max_length} outside [2, {limit}] (the encoder's max_seq_len)")

    def close(self) -> None:
        if self._owns_encoder:
            self.encoder.close()

    def __enter__(self) -> "SparseEncoder":
        return self

    def __exit__(self, *exc) -> None:
        self.close()

    # -- vectors ------------------------------------------------------------------
    def text_ids(self, texts: Sequence[str]) -> List[List[int]]:
        """``[CLS] w.. [SEP]`` per text, at most ``max_length`` tokens (a cut drops the last words, never ``[SEP]``)."""
        out = []
        for t in self.encoder.tokenize(list(texts)):
            ids = [int(v) for v in t]
            out.append(ids if len(ids) <= self.max_length else ids[:self.max_length - 1] + ids[-1:])
        return out

    def _encode_ids(self, ids: List[List[int]], batch_size: int, max_terms: int) -> List[SparseVector]:
        m = int(max_terms)
        if not 1 <= m <= MAX_TERMS:
            raise ValueError(f"max_terms={m} outside [1, {MAX_TERMS}]")
        vecs: List[Optional[SparseVector]] = [None] * len(ids)
        bs = max(1, int(batch_size))
        order = sorted(range(len(ids)), key=lambda i: -len(ids[i]))
        for s in range(0, len(order), bs):
            idx = order[s:s + bs]
            terms, weights, nnz = self.encoder.encode_sparse_ids([ids[i] for i in idx], m)[:3]
            for n, i in enumerate(idx):
                k = min(int(nnz[n]), m)
                vecs[i] = SparseVector(np.array(terms[n, :k], dtype=np.int32), np.array(weights[n, :k], dtype=np.float32))
        return vecs

    def encode(self, texts: Sequence[str], batch_size: int = 32, max_terms: int = 256) -> List[SparseVector]:
        """One ``SparseVector`` per text, in input order: its ``max_terms`` heaviest terms (fewer when fewer are
        positive).  Batches are length-sorted like ``MpnetEncoder.encode``."""
        return self._encode_ids(self.text_ids(texts), batch_size, max_terms)

    def encode_queries(self, texts: Sequence[str], batch_size: int = 32, max_terms: int = 64) -> List[SparseVector]:
        return self.encode(texts, batch_size, max_terms)

    def encode_documents(self, texts: Sequence[str], batch_size: int = 32, max_terms: int = 256) -> List[SparseVector]:
        return self.encode(texts, batch_size, max_terms)

    def score(self, q_vecs: Sequence[SparseVector], d_vecs: Sequence[SparseVector], pairs=None) -> np.ndarray:
        """float32 scores, one per ``(query, doc)`` pair (``None``: all, query-major): the dot product over the shared
        terms, summed in float64 on the host and rounded once (at most 512 entries per side ever leave the device)."""
        if pairs is None:
            pairs = [(i, j) for i in range(len(q_vecs)) for j in range(len(d_vecs))]
        return np.array([sparse_dot_numpy(q_vecs[i], d_vecs[j]) for i, j in pairs], dtype=np.float32)

    # -- CrossEncoder surface -------------------------------------------------------
    def predict(self, pairs: Sequence[Sequence[str]], batch_size: int = 32, activation: Optional[str] = None) -> np.ndarray:
        """float32 scores, one per ``(query, text)`` pair, in input order.  Every distinct query text is encoded once
        (64 terms), every text once per pair (256 terms).  ``activation`` must be ``None`` (a dot product is no logit)."""
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
        q_vecs = self.encode_queries(qtexts, batch_size)
        d_vecs = self.encode_documents([p[1] for p in pairs], batch_size)
        return self.score(q_vecs, d_vecs, [(qindex[p[0]], n) for n, p in enumerate(pairs)])

    def rank(self, query: str, documents: Sequence[str], top_k: Optional[int] = None,
             return_documents: bool = False) -> List[dict]:
        """``[{"corpus_id", "score"[, "text"]}]`` of ``documents`` against ``query``, best first; ties go to the lower
        ``corpus_id``."""
        documents = list(documents)
        return rank_scores(self.predict([(query, d) for d in documents]), documents, top_k, return_documents)

    # -- reading a vector -------------------------------------------------------------
    def _word(self, term: int) -> str:
        vocab = getattr(self.tokenizer, "vocab", None)
        if vocab is None:   # the hashing tokenizer has no word list
            return f"#{int(term)}"
        if getattr(self, "_words", None) is None:
            self._words = {i: w for w, i in vocab.items()}
        return self._words.get(int(term), f"#{int(term)}")

    def decode(self, vec: SparseVector, n: Optional[int] = None) -> List[Tuple[str, float]]:
        """``[(word, weight)]`` of a vector's ``n`` heaviest terms (all of them by default), best first, through the
        tokenizer's vocabulary; with the hashing tokenizer of synthetic weights a word is ``"#<id>"``."""
        k = len(vec.terms) if n is None else max(0, min(int(n), len(vec.terms)))
        return [(self._word(int(t)), float(w)) for t, w in zip(vec.terms[:k], vec.weights[:k])]

    def expansion(self, text: str, n: int = 10) -> List[Tuple[str, float]]:
        """The ``n`` heaviest terms of ``text`` that are not among its own input ids: what the model added."""
        ids = self.text_ids([text])
        vec = self._encode_ids(ids, 1, 256)[0]
        own = np.isin(vec.terms, np.asarray(ids[0], dtype=np.int64))
        return self.decode(SparseVector(vec.terms[~own], vec.weights[~own]), n)
