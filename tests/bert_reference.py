"""TEST SUPPORT, NOT PRODUCT CODE -- plain PyTorch fp32 BERT sentence encoder.

What ``SentenceTransformer("all-MiniLM-L6-v2")`` / ``("BAAI/bge-small-en-v1.5")`` compute: transformers'
``BertModel`` (absolute positions ``0..L-1``, token type 0, post-LN layers with exact-erf GELU) followed by
sentence-transformers' ``Pooling`` (mean over the tokens, or the CLS row) and optionally ``Normalize``.  Weights come
from seeds through ``claude_semantic_search_amd.synth``, bit for bit the tensors ``css_encoder_init_synthetic`` builds
for ``arch = BERT`` (tensor ids as the MPNet oracle's, ``oracle/mpnet_oracle.py``; q / k / v take ids base+0..5 and
token_type_embeddings id 5).  ``tests/golden/make_bert_goldens.py`` checks this restatement against
``transformers.BertModel``; ``tests/test_bert_host.py`` pins it to the committed goldens.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Dict, List, Sequence

import numpy as np
import torch
import torch.nn.functional as F

from claude_semantic_search_amd import synth

CLS_ID, SEP_ID = 101, 102   # bert-base-uncased vocabulary positions of [CLS] / [SEP]


@dataclass
class BertCfg:
    num_layers: int = 6
    hidden: int = 384
    heads: int = 12
    ffn: int = 1536
    vocab: int = 30522
    max_pos: int = 512
    pad_id: int = 0
    max_seq_len: int = 512
    ln_eps: float = 1e-12
    pooling: str = "mean"     # "mean" or "cls"
    normalize: bool = True

    def encoder_overrides(self) -> dict:
        """``cfg_overrides`` of ``MpnetEncoder(synthetic_seed=...)`` for this geometry."""
        return dict(num_layers=self.num_layers, hidden=self.hidden, heads=self.heads, ffn=self.ffn, vocab=self.vocab,
                    max_pos=self.max_pos, rel_buckets=0, pad_id=self.pad_id, max_seq_len=self.max_seq_len,
                    ln_eps=self.ln_eps, arch="bert", pooling=self.pooling, normalize=self.normalize)


SMALL = dict(hidden=384, heads=12, ffn=1536)   # all-MiniLM-L6-v2, bge-small-en-v1.5
BASE = dict(hidden=768, heads=12, ffn=3072)    # bge-base-en-v1.5


def _t(seed: int, tid: int, shape, mean: float, std: float) -> torch.Tensor:
    n = int(np.prod(shape))
    v = synth.normal(synth.tensor_seed(seed, tid), np.arange(n, dtype=np.uint64))
    out = np.float32(mean) + np.float32(std) * v
    return torch.from_numpy(out.astype(np.float32).reshape(shape))


def synth_weights(cfg: BertCfg, seed: int) -> Dict[str, torch.Tensor]:
    """BertModel state dict (no pooler) of the seeded synthetic weights: weights N(0, 0.02^2), biases N(0, 0.05^2),
    LayerNorm gamma N(1, 0.1^2) / beta N(0, 0.05^2); the word-embedding row of the pad id is zero."""
    H, Fd = cfg.hidden, cfg.ffn
    w: Dict[str, torch.Tensor] = {}
    w["embeddings.word_embeddings.weight"] = _t(seed, 0, (cfg.vocab, H), 0.0, 0.02)
    w["embeddings.word_embeddings.weight"][cfg.pad_id] = 0
    w["embeddings.position_embeddings.weight"] = _t(seed, 1, (cfg.max_pos, H), 0.0, 0.02)
    w["embeddings.token_type_embeddings.weight"] = _t(seed, 5, (2, H), 0.0, 0.02)
    w["embeddings.LayerNorm.weight"] = _t(seed, 2, (H,), 1.0, 0.1)
    w["embeddings.LayerNorm.bias"] = _t(seed, 3, (H,), 0.0, 0.05)
    for i in range(cfg.num_layers):
        p, b = f"encoder.layer.{i}.", 16 + 16 * i
        for j, nm in enumerate(("query", "key", "value")):
            w[p + f"attention.self.{nm}.weight"] = _t(seed, b + 2 * j, (H, H), 0.0, 0.02)
            w[p + f"attention.self.{nm}.bias"] = _t(seed, b + 2 * j + 1, (H,), 0.0, 0.05)
        w[p + "attention.output.dense.weight"] = _t(seed, b + 6, (H, H), 0.0, 0.02)
        w[p + "attention.output.dense.bias"] = _t(seed, b + 7, (H,), 0.0, 0.05)
        w[p + "attention.output.LayerNorm.weight"] = _t(seed, b + 8, (H,), 1.0, 0.1)
        w[p + "attention.output.LayerNorm.bias"] = _t(seed, b + 9, (H,), 0.0, 0.05)
        w[p + "intermediate.dense.weight"] = _t(seed, b + 10, (Fd, H), 0.0, 0.02)
        w[p + "intermediate.dense.bias"] = _t(seed, b + 11, (Fd,), 0.0, 0.05)
        w[p + "output.dense.weight"] = _t(seed, b + 12, (H, Fd), 0.0, 0.02)
        w[p + "output.dense.bias"] = _t(seed, b + 13, (H,), 0.0, 0.05)
        w[p + "output.LayerNorm.weight"] = _t(seed, b + 14, (H,), 1.0, 0.1)
        w[p + "output.LayerNorm.bias"] = _t(seed, b + 15, (H,), 0.0, 0.05)
    return w


def synth_batch(cfg: BertCfg, lengths: Sequence[int], seed: int) -> List[List[int]]:
    """Token ids: [CLS] first, [SEP] last, uniform in [999, vocab) between (never the pad id)."""
    batch = []
    for b, L in enumerate(lengths):
        ids = synth.uint(seed, np.arange(L, dtype=np.uint64) + np.uint64(b) * np.uint64(1 << 20), 999, cfg.vocab).tolist()
        ids[0] = CLS_ID
        if L > 1:
            ids[-1] = SEP_ID
        batch.append(ids)
    return batch


def encode_tokens(w: Dict[str, torch.Tensor], cfg: BertCfg, ids: Sequence[int]) -> torch.Tensor:
    """Last hidden state [L, H] of ONE un-padded sequence (token type 0 everywhere)."""
    H, nh = cfg.hidden, cfg.heads
    hd = H // nh
    x_ids = torch.tensor(list(ids), dtype=torch.long)
    L = x_ids.numel()
    x = w["embeddings.word_embeddings.weight"][x_ids] + w["embeddings.token_type_embeddings.weight"][0]
    x = x + w["embeddings.position_embeddings.weight"][:L]
    x = F.layer_norm(x, (H,), w["embeddings.LayerNorm.weight"], w["embeddings.LayerNorm.bias"], cfg.ln_eps)
    for i in range(cfg.num_layers):
        p = f"encoder.layer.{i}."
        lin = lambda t, nm: t @ w[p + nm + ".weight"].T + w[p + nm + ".bias"]  # noqa: E731
        q = lin(x, "attention.self.query").view(L, nh, hd).transpose(0, 1)
        k = lin(x, "attention.self.key").view(L, nh, hd).transpose(0, 1)
        v = lin(x, "attention.self.value").view(L, nh, hd).transpose(0, 1)
        s = q @ k.transpose(1, 2) / math.sqrt(hd)
        c = (torch.softmax(s, dim=-1) @ v).transpose(0, 1).reshape(L, H)
        a = F.layer_norm(lin(c, "attention.output.dense") + x, (H,), w[p + "attention.output.LayerNorm.weight"],
                         w[p + "attention.output.LayerNorm.bias"], cfg.ln_eps)
        y = lin(F.gelu(lin(a, "intermediate.dense")), "output.dense")   # exact erf GELU
        x = F.layer_norm(y + a, (H,), w[p + "output.LayerNorm.weight"], w[p + "output.LayerNorm.bias"], cfg.ln_eps)
    return x


def pool(hs: torch.Tensor, cfg: BertCfg) -> torch.Tensor:
    """sentence-transformers Pooling (mean: sum / max(count, 1e-9); cls: row 0) + optional Normalize."""
    e = hs[0] if cfg.pooling == "cls" else hs.sum(0) / max(float(hs.shape[0]), 1e-9)
    return F.normalize(e, p=2, dim=0, eps=1e-12) if cfg.normalize else e


def encode(w: Dict[str, torch.Tensor], cfg: BertCfg, batch: List[Sequence[int]]) -> np.ndarray:
    """[B, H] float32 sentence embeddings."""
    with torch.no_grad():
        return np.stack([pool(encode_tokens(w, cfg, ids), cfg).numpy() for ids in batch]).astype(np.float32)
