"""``CrossEncoder``: re-ranking with a BERT cross-encoder on the GPU encoder, in the shape of
``sentence_transformers.CrossEncoder`` (``predict`` / ``rank``).

A cross-encoder reads ``[CLS] query [SEP] text [SEP]`` in ONE forward pass and returns one relevance logit per pair
(transformers' ``BertForSequenceClassification`` with one label: the ``cross-encoder/ms-marco-MiniLM-L-*`` family).
The body is the BERT encoder of ``MpnetEncoder`` with token type 1 on the second segment; the head (pooler dense + tanh,
classifier) runs on the device in fp32 (``css_encoder_set_head`` / ``css_encoder_forward_pairs``).

Pair building is transformers' ``tokenizer(a, b, truncation=True, max_length=L)``: each side is WordPiece-tokenised
without special tokens and the pair is cut with the ``longest_first`` rule (``build_pair``).
"""
from __future__ import annotations

import json
from pathlib import Path
from typing import Dict, List, Optional, Sequence, Tuple, Union

import numpy as np

from . import synth
from .mpnet_encoder import BERT_SMALL_CFG, MpnetEncoder, _find_model_dir, _load_state_dict, parse_model_config

#: synthetic tensor ids of the head (the body uses 0-5 and 16 + 16 * layer + 0..15): (id, std) of pooler weight,
#: pooler bias, classifier weight, classifier bias
HEAD_SYNTH = {"pooler_w": (6, 0.02), "pooler_b": (7, 0.05), "cls_w": (8, 0.05), "cls_b": (9, 0.05)}

_HEAD_KEYS = ("pooler.dense.weight", "pooler.dense.bias", "classifier.weight", "classifier.bias")


def build_pair(a_ids: Sequence[int], b_ids: Sequence[int], cls: int, sep: int, max_length: int) -> Tuple[List[int], int]:
    """``([CLS] a [SEP] b [SEP], seg_start)`` with ``seg_start = len(a) + 2`` (the first type-1 position) after
    transformers' ``longest_first`` truncation to ``max_length`` tokens: while the pair is too long, drop the last
    token of ``a`` if ``len(a) > len(b)``, else of ``b``."""
    if max_length < 3:
        raise ValueError(f"build_pair: max_length={max_length} leaves no room for [CLS] a [SEP] b [SEP]")
    a, b = [int(t) for t in a_ids], [int(t) for t in b_ids]
    over = len(a) + len(b) + 3 - int(max_length)
    for _ in range(max(0, over)):
        if len(a) > len(b):
            a.pop()
        else:
            b.pop()
    return [cls] + a + [sep] + b + [sep], len(a) + 2


def parse_cross_encoder_config(model_dir: Union[str, Path]) -> dict:
    """The encoder configuration of a cross-encoder checkpoint directory (no GPU needed).  Refuses, with a ``ValueError``
    naming the field: a ``model_type`` other than ``bert``, anything but exactly one label (``num_labels`` /
    ``id2label``), an ``hidden_act`` other than ``gelu`` and a geometry the encoder refuses (``parse_model_config``)."""
    model_dir = Path(model_dir)
    hf = json.loads((model_dir / "config.json").read_text())
    model_type = hf.get("model_type")
    if model_type != "bert":
        raise ValueError(f"unsupported model_type {model_type!r} for a cross-encoder (supported: 'bert')")
    if "num_labels" in hf:
        n_labels, field = int(hf["num_labels"]), "num_labels"
    elif hf.get("id2label") is not None:
        n_labels, field = len(hf["id2label"]), "id2label"
    else:
        n_labels, field = 2, "num_labels"   # (transformers' default when neither is written)
    if n_labels != 1:
        raise ValueError(f"unsupported {field}: {n_labels} labels (a re-ranking cross-encoder has exactly one)")
    if hf.get("id2label") is not None and len(hf["id2label"]) != 1:
        raise ValueError(f"unsupported id2label: {len(hf['id2label'])} labels (a re-ranking cross-encoder has exactly one)")
    cfg = parse_model_config(model_dir)   # hidden_act, hidden_size, head_dim, type_vocab_size, position_embedding_type
    cfg.update(pooling="cls", normalize=False)
    return cfg


def split_state_dict(sd: Dict[str, np.ndarray]) -> Tuple[Dict[str, np.ndarray], Dict[str, np.ndarray]]:
    """``(body, head)`` of a ``BertForSequenceClassification`` state dict: ``[bert.]pooler.dense.{weight,bias}`` and
    ``classifier.{weight,bias}`` form the head, everything else the body.  A checkpoint without them raises: it is a
    sentence encoder, not a cross-encoder."""
    body: Dict[str, np.ndarray] = {}
    head: Dict[str, np.ndarray] = {}
    for k, v in sd.items():
        name = k[5:] if k.startswith("bert.") else k
        if name in _HEAD_KEYS:
            if name in head:
                raise ValueError(f"cross-encoder checkpoint names '{name}' more than once")
            head[name] = v
        else:
            body[k] = v
    missing = [k for k in _HEAD_KEYS if k not in head]
    if missing:
        raise ValueError(f"checkpoint has no {', '.join(missing)}: a sentence encoder, not a cross-encoder "
                         "(BertForSequenceClassification keeps bert.pooler.dense.* and classifier.*)")
    return body, head


def synth_head(hidden: int, seed: int) -> Dict[str, np.ndarray]:
    """The seeded synthetic head, formed on the host with ``synth``: pooler weight N(0, 0.02^2), pooler bias
    N(0, 0.05^2), classifier weight N(0, 0.05^2), classifier bias N(0, 0.05^2) (tensor ids ``HEAD_SYNTH``)."""
    def t(key, n):
        tid, std = HEAD_SYNTH[key]
        v = synth.normal(synth.tensor_seed(seed, tid), np.arange(n, dtype=np.uint64))
        return (np.float32(std) * v).astype(np.float32)

    return {"pooler_w": t("pooler_w", hidden * hidden).reshape(hidden, hidden), "pooler_b": t("pooler_b", hidden),
            "cls_w": t("cls_w", hidden), "cls_b": t("cls_b", 1)}


def rank_scores(scores: Sequence[float], documents: Optional[Sequence[str]] = None, top_k: Optional[int] = None,
                return_documents: bool = False) -> List[dict]:
    """``[{"corpus_id", "score"[, "text"]}]`` best first; ties go to the lower ``corpus_id``."""
    s = np.asarray(scores, dtype=np.float32)
    order = np.argsort(-s, kind="stable")
    if top_k is not None:
        order = order[:max(0, int(top_k))]
    out = []
    for i in order:
        hit = {"corpus_id": int(i), "score": float(s[i])}
        if return_documents:
            hit["text"] = documents[int(i)]
        out.append(hit)
    return out


class CrossEncoder:
    def __init__(self, model_name_or_path: Optional[str], device: int = 0, compute: str = "bf16",
                 max_length: Optional[int] = None, synthetic_seed: Optional[int] = None,
                 cfg_overrides: Optional[dict] = None):
        self.model_dir = None
        if synthetic_seed is None:
            model_dir = _find_model_dir(model_name_or_path or "", None)
            if model_dir is None:
                raise FileNotFoundError(f"model '{model_name_or_path}' not found locally (no network): pass a directory "
                                        "in HF layout, or synthetic_seed=<int> for seeded synthetic weights")
            cfg = parse_cross_encoder_config(model_dir)
            body, head = split_state_dict(_load_state_dict(model_dir))
            over = dict(pooling=cfg["pooling"], normalize=cfg["normalize"])
            over.update(cfg_overrides or {})
            self.encoder = MpnetEncoder(str(model_dir), device=device, compute=compute, cfg_overrides=over, weights=body)
            try:
                self.encoder.set_head(head["pooler.dense.weight"], head["pooler.dense.bias"],
                                      head["classifier.weight"], head["classifier.bias"])
                if self.encoder.tokenizer is None:
                    raise FileNotFoundError(self.encoder.tokenizer_problem)
            except Exception:
                self.encoder.close()
                raise
            self.tokenizer = self.encoder.tokenizer
            self.model_dir = model_dir
        else:
            cfg = dict(BERT_SMALL_CFG, pooling="cls", normalize=False)
            if cfg_overrides:
                cfg.update(cfg_overrides)
            if cfg.get("arch") != "bert":
                raise ValueError(f"unsupported arch {cfg.get('arch')!r} for a cross-encoder (supported: 'bert')")
            self.encoder = MpnetEncoder(synthetic_seed=synthetic_seed, device=device, compute=compute, cfg_overrides=cfg)
            h = synth_head(int(cfg["hidden"]), synthetic_seed)
            self.encoder.set_head(h["pooler_w"], h["pooler_b"], h["cls_w"], h["cls_b"])
            self.tokenizer = self.encoder.tokenizer   # (HashTokenizer: any deterministic text -> ids map will do)
        self.cfg = self.encoder.cfg
        limit = int(self.cfg["max_seq_len"])
        self.max_length = limit if max_length is None else int(max_length)
        if not 3 <= self.max_length <= limit:
            self.encoder.close()
            raise ValueError(f"max_length={self.max_length} outside [3, {limit}] (the encoder's max_seq_len)")
        if synthetic_seed is None:
            self.cls_id, self.sep_id = int(self.tokenizer.bos), int(self.tokenizer.eos)
        else:   # the hashing tokenizer has no [CLS] / [SEP]: bert-base-uncased's positions (never the pad id 0)
            self.cls_id, self.sep_id = (101, 102) if int(self.cfg["vocab"]) > 102 else (1, 2)

    def close(self) -> None:
        self.encoder.close()

    def __enter__(self) -> "CrossEncoder":
        return self

    def __exit__(self, *exc) -> None:
        self.close()

    # -- pairs ----------------------------------------------------------------
    def _side_ids(self, texts: Sequence[str]) -> List[List[int]]:
        """WordPiece ids without special tokens, at most ``max_length`` per text (a side never keeps more)."""
        L = self.max_length + 2
        if hasattr(self.tokenizer, "encode_batch"):
            toks = self.tokenizer.encode_batch(list(texts), L)
        else:
            toks = [self.tokenizer.encode(t, L) for t in texts]
        return [[int(v) for v in t[1:-1]] for t in toks]

    def tokenize_pairs(self, pairs: Sequence[Sequence[str]]) -> Tuple[List[List[int]], List[int]]:
        """``(ids, seg_starts)`` of ``[CLS] a [SEP] b [SEP]`` for every ``(a, b)``, truncated to ``max_length``."""
        a = self._side_ids([p[0] for p in pairs])
        b = self._side_ids([p[1] for p in pairs])
        built = [build_pair(x, y, self.cls_id, self.sep_id, self.max_length) for x, y in zip(a, b)]
        return [ids for ids, _ in built], [seg for _, seg in built]

    def predict(self, pairs: Sequence[Sequence[str]], batch_size: int = 32, activation: Optional[str] = None) -> np.ndarray:
        """float32 logits, one per ``(query, text)`` pair, in input order.  ``activation="sigmoid"`` maps them to
        (0, 1) on the host.  Batches are length-sorted like ``MpnetEncoder.encode``."""
        if activation not in (None, "sigmoid"):
            raise ValueError(f"unsupported activation {activation!r} (supported: None, 'sigmoid')")
        pairs = list(pairs)
        if not pairs:
            return np.zeros(0, dtype=np.float32)
        ids, seg = self.tokenize_pairs(pairs)
        out = np.empty(len(pairs), dtype=np.float32)
        bs = max(1, int(batch_size))
        order = sorted(range(len(ids)), key=lambda i: -len(ids[i]))
        for s in range(0, len(order), bs):
            idx = order[s:s + bs]
            out[idx] = self.encoder.score_pair_ids([ids[i] for i in idx], [seg[i] for i in idx])
        if activation == "sigmoid":
            out = (1.0 / (1.0 + np.exp(-out.astype(np.float64)))).astype(np.float32)
        return out

    def rank(self, query: str, documents: Sequence[str], top_k: Optional[int] = None,
             return_documents: bool = False) -> List[dict]:
        """``[{"corpus_id", "score"[, "text"]}]`` of ``documents`` against ``query``, best first; ties go to the lower
        ``corpus_id``."""
        documents = list(documents)
        return rank_scores(self.predict([(query, d) for d in documents]), documents, top_k, return_documents)
