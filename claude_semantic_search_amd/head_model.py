"""``HeadModel``: what ``CrossEncoder``, ``SparseEncoder`` and ``LateInteraction`` share.  Each is a BERT body on
``MpnetEncoder`` plus a head; the base opens the encoder (checkpoint directory or seeded synthetic weights), attaches
the head, and carries ``close`` / ``with`` / ``rank``.  A subclass supplies its config parser, its state-dict splitter,
its synthetic head, how a head is attached, and ``predict``.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from .mpnet_encoder import BERT_SMALL_CFG, MpnetEncoder, _find_model_dir, _load_state_dict


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


def distinct_queries(pairs: Sequence[Sequence[str]]) -> Tuple[List[str], Dict[str, int]]:
    """``(texts, index)``: every distinct query text of ``(query, text)`` pairs once, in order of first use, and the
    position of each text in that list (a ``predict`` encodes each query once, however many pairs name it)."""
    texts: List[str] = []
    index: Dict[str, int] = {}
    for p in pairs:
        if p[0] not in index:
            index[p[0]] = len(texts)
            texts.append(p[0])
    return texts, index


class HeadModel:
    """A subclass defines ``_parse_config(model_dir) -> cfg`` (its ``parse_*_config``), ``_split(state_dict, cfg) ->
    (body, head)``, ``_synth(cfg, seed) -> head``, ``_attach(head)`` (hands either head to ``self.encoder``) and
    ``predict(pairs)``."""
    #: the model kind as the arch error text names it ("unsupported arch 'mpnet' for <noun> (supported: 'bert')")
    _noun = ""
    #: pooling / normalize of the synthetic encoder (a checkpoint's come from ``_parse_config``)
    _pooling, _normalize = "cls", False

    def __init__(self, model_name_or_path: Optional[str], device: int, compute: str, synthetic_seed: Optional[int],
                 cfg_overrides: Optional[dict], encoder=None):
        # encoder: an object with the subclass's surface of MpnetEncoder (tests pass a fake; no GPU is touched)
        self.model_dir = None
        self._owns_encoder = encoder is None      # a caller's encoder stays the caller's: close() leaves it open
        if encoder is not None:
            self.encoder = encoder
        else:
            model_dir = None
            if synthetic_seed is None:
                model_dir = _find_model_dir(model_name_or_path or "", None)
                if model_dir is None:
                    raise FileNotFoundError(f"model '{model_name_or_path}' not found locally (no network): pass a "
                                            "directory in HF layout, or synthetic_seed=<int> for seeded synthetic weights")
                cfg = self._parse_config(model_dir)
                body, head = self._split(_load_state_dict(model_dir), cfg)
                over = dict(pooling=cfg["pooling"], normalize=cfg["normalize"])
                over.update(cfg_overrides or {})
                self.encoder = MpnetEncoder(str(model_dir), device=device, compute=compute, cfg_overrides=over, weights=body)
            else:
                cfg = dict(BERT_SMALL_CFG, pooling=self._pooling, normalize=self._normalize)
                if cfg_overrides:
                    cfg.update(cfg_overrides)
                if cfg.get("arch") != "bert":
                    raise ValueError(f"unsupported arch {cfg.get('arch')!r} for {self._noun} (supported: 'bert')")
                self.encoder = MpnetEncoder(synthetic_seed=synthetic_seed, device=device, compute=compute, cfg_overrides=cfg)
                head = self._synth(cfg, synthetic_seed)
            try:
                self._attach(head)
                # (synthetic weights come with the hashing tokenizer: any deterministic text -> ids map will do)
                if self.encoder.tokenizer is None:
                    raise FileNotFoundError(self.encoder.tokenizer_problem)
            except Exception:
                self.encoder.close()
                raise
            self.model_dir = model_dir
        self.cfg = self.encoder.cfg
        self.tokenizer = self.encoder.tokenizer

    def close(self) -> None:
        if self._owns_encoder:
            self.encoder.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc) -> None:
        self.close()

    def rank(self, query: str, documents: Sequence[str], top_k: Optional[int] = None,
             return_documents: bool = False) -> List[dict]:
        """``[{"corpus_id", "score"[, "text"]}]`` of ``documents`` against ``query``, best first; ties go to the lower
        ``corpus_id``."""
        documents = list(documents)
        return rank_scores(self.predict([(query, d) for d in documents]), documents, top_k, return_documents)
