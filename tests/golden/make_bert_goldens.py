"""Generates tests/golden/bert_*.npz.

    python tests/golden/make_bert_goldens.py

The expected embeddings come from the in-container ``transformers.BertModel`` (5.15.0: the architecture of
all-MiniLM-L6-v2 and bge-*-en-v1.5) with the seeded synthetic weights of ``tests/bert_reference.py`` loaded through
``load_state_dict``, a padded batch with its attention mask and token type 0, then sentence-transformers' ``Pooling``
(mean over the unmasked tokens, or the CLS row) + ``Normalize`` restated on the HF output.  ``tests/bert_reference.py``
is run next to it and must agree to 2e-6.

bert_small_2layer.npz: hidden 384, 12 heads x 32, ffn 1536 (MiniLM / bge-small geometry), 2 layers.
bert_base_2layer.npz:  hidden 768, 12 heads x 64, ffn 3072 (bge-base geometry), 2 layers.
Each holds ``emb_mean`` and ``emb_cls`` [8, H] for lengths {1, 2, 7, 31, 128, 255, 383, 384}, weights seed 7, token
seed 11.  Inputs are regenerated from the seeds at test time; only outputs are stored.
"""
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import bert_reference as br  # noqa: E402

OUT = Path(__file__).resolve().parent
LENGTHS = [1, 2, 7, 31, 128, 255, 383, 384]
WSEED, BSEED = 7, 11


def hf_model(cfg: br.BertCfg, w):
    from transformers import BertConfig, BertModel

    hf = BertModel(BertConfig(vocab_size=cfg.vocab, hidden_size=cfg.hidden, num_hidden_layers=cfg.num_layers,
                              num_attention_heads=cfg.heads, intermediate_size=cfg.ffn, hidden_act="gelu",
                              max_position_embeddings=cfg.max_pos, type_vocab_size=2, layer_norm_eps=cfg.ln_eps,
                              pad_token_id=cfg.pad_id, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0),
                   add_pooling_layer=False).eval()
    missing, unexpected = hf.load_state_dict(w, strict=False)
    assert not unexpected and all("position_ids" in m or "token_type_ids" in m for m in missing), (missing, unexpected)
    return hf


def hf_encode(cfg: br.BertCfg, w, batch, chunk=4) -> np.ndarray:
    """transformers forward on padded batches + Pooling(mean | cls) + Normalize."""
    hf = hf_model(cfg, w)
    outs = []
    for c0 in range(0, len(batch), chunk):
        part = batch[c0:c0 + chunk]
        Lmax = max(len(s) for s in part)
        ids = torch.full((len(part), Lmax), cfg.pad_id, dtype=torch.long)
        mask = torch.zeros((len(part), Lmax), dtype=torch.long)
        for b, s in enumerate(part):
            ids[b, :len(s)] = torch.tensor(s)
            mask[b, :len(s)] = 1
        with torch.no_grad():
            hs = hf(input_ids=ids, attention_mask=mask, token_type_ids=torch.zeros_like(ids)).last_hidden_state
        if cfg.pooling == "cls":
            e = hs[:, 0]
        else:
            m = mask[:, :, None].float()
            e = (hs * m).sum(1) / m.sum(1).clamp(min=1e-9)
        if cfg.normalize:
            e = torch.nn.functional.normalize(e, p=2, dim=1, eps=1e-12)
        outs.append(e.numpy())
    return np.concatenate(outs).astype(np.float32)


def main():
    for name, geo in (("bert_small_2layer", br.SMALL), ("bert_base_2layer", br.BASE)):
        cfg = br.BertCfg(num_layers=2, **geo)
        w = br.synth_weights(cfg, WSEED)
        batch = br.synth_batch(cfg, LENGTHS, BSEED)
        res = {}
        for pooling in ("mean", "cls"):
            cfg.pooling = pooling
            emb = hf_encode(cfg, w, batch)
            ref = br.encode(w, cfg, batch)
            err = np.abs(emb - ref).max()
            assert err <= 2e-6, (name, pooling, err)
            print(f"{name} {pooling}: |transformers - bert_reference| = {err:.2e}")
            res["emb_" + pooling] = emb
        np.savez_compressed(OUT / f"{name}.npz", lengths=np.array(LENGTHS, np.int32), wseed=WSEED, bseed=BSEED,
                            num_layers=2, **res)


if __name__ == "__main__":
    main()
